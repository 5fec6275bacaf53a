"""Golden answer of the UNMODIFIED reference for tests/test_sampling.py::test_reference_likelihood_weighting_converges_to_the_enumerated_limit:
its likelihood-weighting estimate of P(Rain | Sprinkler=True) on the sprinkler example, 6 000 iterations, the reference's own random
stream seeded 5 (with oracle/refload.py's stand-in for `vose`, which this path does not call).  Where the reference is present:

    python tests/golden/make_likelihood_sprinkler.py

writes tests/golden/likelihood_sprinkler.json: the request and the estimate as [label, probability as float.hex()] pairs."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import netspec  # noqa: E402
from oracle import refload  # noqa: E402

QUERY, EVENT, N_ITERATIONS, SEED = "Rain", {"Sprinkler": True}, 6000, 5


def main():
    ref = refload.load().examples.sprinkler()
    ref._rng.seed(SEED)
    got = ref.query(QUERY, event=EVENT, algorithm="likelihood", n_iterations=N_ITERATIONS)
    netspec.save(os.path.join(HERE, "likelihood_sprinkler.json"),
                 {"network": "sprinkler", "query": QUERY, "event": EVENT, "n_iterations": N_ITERATIONS, "seed": SEED,
                  "estimate": [[netspec._py(lab), float(p).hex()] for lab, p in got.items()]})


if __name__ == "__main__":
    main()
