"""Structure learning: the mirror of sorobn/structure.py (`chow_liu`) and, beyond the reference, score-based search
(`hill_climb`, `family_scores`), exact search for up to 24 columns (`exact_search`, `best_dag`), constraint-based search
(`pc`, `ci_tests`), bootstrap arc strengths (`bootstrap`) and exact arc posteriors over all DAGs (`arc_posteriors`,
`arc_posteriors_from_scores`); see learning.py."""
from .learning import (ArcPosterior, ArcStrength, PCResult, arc_posteriors, arc_posteriors_from_scores, best_dag, bootstrap, chi2_sf,
                       chow_liu, ci_tests, exact_search, family_scores, hill_climb, mutual_information, pc)

__all__ = ["chow_liu", "mutual_information", "hill_climb", "family_scores", "pc", "ci_tests", "chi2_sf", "PCResult", "bootstrap",
           "ArcStrength", "exact_search", "best_dag", "arc_posteriors", "arc_posteriors_from_scores", "ArcPosterior"]
