"""Structure learning: the mirror of sorobn/structure.py (`chow_liu`) and, beyond the reference, score-based search
(`hill_climb`, `family_scores`); see learning.py."""
from .learning import chow_liu, family_scores, hill_climb, mutual_information

__all__ = ["chow_liu", "mutual_information", "hill_climb", "family_scores"]
