"""Structure learning: the mirror of sorobn/structure.py (`chow_liu`) and, beyond the reference, score-based search
(`hill_climb`, `family_scores`), exact search for up to 24 columns (`exact_search`, `best_dag`), constraint-based search
(`pc`, `ci_tests`) and bootstrap arc strengths (`bootstrap`); see learning.py."""
from .learning import (ArcStrength, PCResult, best_dag, bootstrap, chi2_sf, chow_liu, ci_tests, exact_search, family_scores, hill_climb,
                       mutual_information, pc)

__all__ = ["chow_liu", "mutual_information", "hill_climb", "family_scores", "pc", "ci_tests", "chi2_sf", "PCResult", "bootstrap",
           "ArcStrength", "exact_search", "best_dag"]
