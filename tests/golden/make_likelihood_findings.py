"""Golden answers of the UNMODIFIED reference for likelihood findings (tests/test_likelihood_host.py, tests/test_likelihood.py).

The reference has no soft evidence, but it computes the same posterior on an AUGMENTED network: every finding variable X gets a
binary child V with P(V = 1 | X = x) = lambda(x) / max lambda, and V = 1 is observed (tests/likelihood_check.py augment).  Where the
reference is present:

    PYTHONHASHSEED=0 python tests/golden/make_likelihood_findings.py

writes tests/golden/likelihood_findings.json: per network how to rebuild it (an example by name, or a generator recipe pinned by the
sum of its CPT numbers), and per request the query, the hard evidence, the findings as [label, weight] pairs and the reference's
answer on the augmented network in the format of make_golden.py (values as float.hex()).

Networks: Asia, sprinkler, a 3 x 3 three-state grid and a random DAG with sparse CPTs.  Findings on roots, leaves and inner nodes, one to
three per request, with and without hard evidence; some requests carry a finding on their query variable - the augmented query is
still valid there, because V is the evidence, not X."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pandas as pd  # noqa: E402

import golden_util as gu  # noqa: E402
import likelihood_check as lc  # noqa: E402
import netspec  # noqa: E402
from oracle import refload  # noqa: E402

assert os.environ.get("PYTHONHASHSEED") == "0", "run with PYTHONHASHSEED=0"

DAG = dict(seed=32, n_nodes=8, max_parents=2, cards=(2, 3, 4), p_zero=0.08, p_missing=0.1)
GRID = dict(R=3, C=3, K=3, seed=4)


def cpt_sum_hex(spec):
    return float(sum(row[-1] for c in spec["cpts"].values() for row in c["rows"])).hex()


def series_to_json(s):
    idx = s.index
    rows = [list(map(netspec._py, k if isinstance(k, tuple) else (k,))) for k in idx.tolist()]
    return {"name": s.name, "index_names": [str(n) for n in idx.names], "index": rows, "multi": isinstance(idx, pd.MultiIndex),
            "values_hex": [float(v).hex() for v in s.tolist()]}


def w(labels, *weights):
    return [[lab, float(x)] for lab, x in zip(labels, weights)]


T, F = True, False
ASIA = [
    # (query, event, findings): root, inner and leaf findings; one to three; with and without hard evidence
    (["Lung cancer"], [["Smoker", T]], {"Positive X-ray": w([F, T], 0.2, 0.9), "Visit to Asia": w([F, T], 1.0, 3.0)}),
    (["Tuberculosis"], [], {"Smoker": w([F, T], 0.3, 0.7)}),
    (["Bronchitis", "Lung cancer"], [["Visit to Asia", F]], {"Dispnea": w([F, T], 0.1, 0.8), "TB or cancer": w([F, T], 2.0, 0.5),
                                                             "Smoker": w([F, T], 0.6, 0.4)}),
    (["Dispnea"], [], {"Dispnea": w([F, T], 0.25, 0.75)}),                      # the finding on the query variable
    (["Smoker"], [["Dispnea", T]], {"Smoker": w([F, T], 5.0, 1.0), "Positive X-ray": w([F, T], 0.0, 1.0)}),  # a hard zero: "X-ray is not False"
    (["TB or cancer"], [], {"Tuberculosis": w([F, T], 1.0, 40.0)}),
]
SPRINKLER = [
    (["Rain"], [], {"Wet grass": w([F, T], 0.1, 0.9)}),
    (["Cloudy"], [["Sprinkler", T]], {"Wet grass": w([F, T], 0.3, 0.6), "Rain": w([F, T], 0.8, 0.2)}),
    (["Sprinkler", "Rain"], [], {"Cloudy": w([F, T], 0.5, 2.0), "Rain": w([F, T], 1.0, 0.25)}),
]
GRID_REQS = [
    (["004"], [], {"000": w(range(3), 0.2, 0.5, 0.3)}),
    (["008"], [["000", 1]], {"004": w(range(3), 1.0, 0.0, 2.0), "002": w(range(3), 0.3, 0.3, 0.9)}),
    (["000", "008"], [["006", 2]], {"008": w(range(3), 0.7, 0.1, 0.2), "004": w(range(3), 0.4, 0.4, 0.2), "001": w(range(3), 0.0, 1.0, 1.0)}),
    (["003"], [], {"008": w(range(3), 0.05, 0.9, 0.05)}),
]


def dag_requests(spec):
    dom = netspec.domains(spec)
    nodes = spec["nodes"]
    lam = lambda n, *x: w(dom[n], *x[:len(dom[n])])
    return [
        ([nodes[5]], [], {nodes[0]: lam(nodes[0], 0.3, 1.2, 0.5, 0.9)}),
        ([nodes[2]], [[nodes[6], dom[nodes[6]][0]]], {nodes[7]: lam(nodes[7], 0.9, 0.1, 0.4, 0.2), nodes[3]: lam(nodes[3], 1.0, 2.0, 0.0, 0.5)}),
        ([nodes[7], nodes[1]], [[nodes[0], dom[nodes[0]][-1]]], {nodes[7]: lam(nodes[7], 0.2, 0.7, 0.6, 0.1), nodes[4]: lam(nodes[4], 0.5, 0.25, 1.0, 0.3),
                                                                 nodes[2]: lam(nodes[2], 1.5, 0.5, 0.75, 0.1)}),
        ([nodes[4]], [], {nodes[4]: lam(nodes[4], 0.6, 0.3, 0.8, 0.2)}),
    ]


def run(sorobn, spec, reqs):
    wrap = refload.HashedName if spec["hashed_names"] else (lambda s: s)
    out = []
    for q, ev, findings in reqs:
        aug, add, _ = lc.augment(spec, {n: dict((lab, x) for lab, x in pairs) for n, pairs in findings.items()})
        bn = netspec.build(aug, sorobn.BayesNet, wrap=wrap if spec["hashed_names"] else None)
        event = {wrap(k): v for k, v in ev}
        event.update({wrap(k): v for k, v in add.items()})
        ans = bn.query(*[wrap(x) for x in q], event=event)
        out.append({"query": list(q), "event": [[k, netspec._py(v)] for k, v in ev],
                    "findings": {n: [[netspec._py(lab), x] for lab, x in pairs] for n, pairs in findings.items()},
                    "expect": series_to_json(ans)})
    return out


def main():
    sorobn = refload.load()
    examples = {e["spec"]["name"]: e["spec"] for e in gu.load("examples.json")}
    nets = []
    for name, reqs in (("asia", ASIA), ("sprinkler", SPRINKLER)):
        nets.append({"net": {"kind": "example", "name": name}, "requests": run(sorobn, examples[name], reqs)})
    grid = netspec.grid_spec(GRID["R"], GRID["C"], GRID["K"], seed=GRID["seed"])
    nets.append({"net": {"kind": "grid", **GRID, "cpt_sum_hex": cpt_sum_hex(grid)}, "requests": run(sorobn, grid, GRID_REQS)})
    dag = netspec.random_dag_spec(**DAG)
    nets.append({"net": {"kind": "dag", **{k: (list(v) if isinstance(v, tuple) else v) for k, v in DAG.items()}, "cpt_sum_hex": cpt_sum_hex(dag)},
                 "requests": run(sorobn, dag, dag_requests(dag))})
    netspec.save(os.path.join(HERE, "likelihood_findings.json"), nets)
    print(sum(len(n["requests"]) for n in nets), "requests")


if __name__ == "__main__":
    main()
