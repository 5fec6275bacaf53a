"""Plain numpy twin of likelihood findings (Pearl's virtual evidence; tests/test_likelihood.py, tests/test_likelihood_host.py): the
joint of a small network - the CPTs of the relevant variables, sliced by the hard evidence - multiplied by one weight vector per
finding variable, by enumeration over the flattened network (sorobn_amd.flatten), i.e. the tables the engine itself is given; then
the posterior, the mass, the argmax and the marginal MAP of it.  `augment` builds the network on which the UNMODIFIED reference
computes the same thing - every finding variable X gets a binary child V, P(V = 1 | X = x) = lambda(x) / max lambda, observed at 1 -
and the runners of the host interpreter (tools/prog_sim.cpp --lh) are here too.

A request's findings are a list [(variable id, weights float64[card])] in the order the caller gives them."""
import copy
import os
import subprocess

import numpy as np

import map_check as mp
import mpe_check as mc
import sim_tools

ROOT = mc.ROOT


def weighted_joint(f, ev, findings, rel=None):
    """-> (axis variable ids ascending, table): prod of the CPTs of `rel` (None: every variable) sliced by ev, times the weights."""
    fs = [t for v, t in enumerate(mc._sliced(f, ev)) if rel is None or v in rel]
    for v, w in findings:
        w = np.asarray(w, np.float64)
        assert len(w) == f.card[v] and v not in ev
        fs.append(([int(v)], w))
    return mc._mul(fs)


def _relevant(f, q, ev, findings):
    return mp.relevant(f, list(q) + list(ev) + [v for v, _ in findings])


def mass(f, q, ev, findings, prune=True):
    """The unnormalised table over q (C-order, caller's order; one cell for q = ()) of the weighted joint: MIBN_Q_UNNORMALISED.
    prune: only the CPTs of the query, evidence and finding variables and of their ancestors take part."""
    if any(c < 0 or c >= f.card[v] for v, c in ev.items()):
        return np.zeros(int(np.prod([int(f.card[v]) for v in q])))
    vs, a = weighted_joint(f, ev, findings, _relevant(f, q, ev, findings) if prune else None)
    drop = tuple(i for i, v in enumerate(vs) if v not in q)
    s = a.sum(axis=drop) if drop else a
    rest = [v for v in vs if v in q]
    s = np.transpose(s, [rest.index(v) for v in q]) if q else s
    return np.asarray(s, np.float64).reshape(-1)


def posterior(f, q, ev, findings, prune=True):
    """mass / its sum; all zero where nothing has positive mass."""
    m = mass(f, q, ev, findings, prune)
    z = m.sum()
    return m / z if z > 0 else np.zeros_like(m)


def _best(table, vs):
    flat = table.reshape(-1)
    order = np.argsort(-flat, kind="stable")
    p1 = float(flat[order[0]])
    p2 = float(flat[order[1]]) if flat.size > 1 else 0.0
    best = np.unravel_index(int(order[0]), table.shape) if table.ndim else ()
    return p1, p2, dict(zip(vs, (int(c) for c in best)))


def mpe(f, ev, findings):
    """-> (log_p, codes [n] - evidence keeps its codes, -1 everywhere else at zero mass -, p1, p2): the argmax of the weighted joint
    of EVERY CPT (an MPE never prunes), the first maximum in C order (ties go to the lowest codes), and the runner-up."""
    n = len(f.card)
    vs, a = weighted_joint(f, ev, findings)
    p1, p2, at = _best(a, vs)
    codes = np.full(n, -1, np.int64)
    for v, c in ev.items():
        codes[v] = c
    if p1 <= 0:
        return -np.inf, codes, p1, p2
    for v in range(n):
        if v not in ev:
            codes[v] = at.get(v, 0)
    return float(np.log(p1)), codes, p1, p2


def marginal_map(f, mvars, ev, findings, prune=False):
    """-> (log_p, codes in the order of mvars, p1, p2): max_m sum_h of the weighted joint."""
    rel = _relevant(f, mvars, ev, findings) if prune else None
    vs, a = weighted_joint(f, ev, findings, rel)
    ms = set(int(v) for v in mvars)
    drop = tuple(i for i, v in enumerate(vs) if v not in ms)
    table = a.sum(axis=drop) if drop else a
    p1, p2, at = _best(np.asarray(table), [v for v in vs if v in ms])
    if p1 <= 0:
        return -np.inf, [-1] * len(mvars), p1, p2
    return float(np.log(p1)), [at.get(int(v), 0) for v in mvars], p1, p2


# ------------------------------------------------------------------------------------------------------- the augmented network
def augment(spec, findings):
    """findings: {variable name: {label: weight}} (a label of the domain that is not named weighs 0) -> (spec of the augmented
    network, the event to add, sum of log max lambda).  Every finding variable X gets a binary child V with the CPT
    [1 - lambda(x) / max lambda, lambda(x) / max lambda]; observing V = 1 multiplies the joint by lambda / max lambda, which leaves
    every normalised answer as it is and takes `sum log max lambda` off every log mass."""
    out = copy.deepcopy(spec)
    dom = _domains(spec)
    numeric = all(n.isdigit() for n in spec["nodes"])
    event, log_scale = {}, 0.0
    for k, (name, lam) in enumerate(findings.items()):
        child = f"{len(spec['nodes']) + k:03d}" if numeric else f"V({name})"
        assert child not in out["nodes"]
        top = max(float(lam.get(lab, 0.0)) for lab in dom[name])
        assert top > 0, "a finding that is zero everywhere has no augmented network"
        rows = []
        for lab in dom[name]:
            p = float(lam.get(lab, 0.0)) / top
            rows += [[lab, 0, 1.0 - p], [lab, 1, p]]
        out["nodes"].append(child)
        out["edges"].append([name, child])
        out["cpts"][child] = {"names": [name, child], "rows": rows}
        event[child] = 1
        log_scale += float(np.log(top))
    out["name"] = spec["name"] + "+findings"
    return out, event, log_scale


def _domains(spec):
    import netspec
    return netspec.domains(spec)


def encode(f, findings):
    """{name: {label: weight}} -> [(id, weights)] over a FlatNetwork, like Backend.encode_likelihood."""
    out = []
    for name, lam in findings.items():
        v = f.id[name]
        w = np.zeros(int(f.card[v]))
        for lab, x in lam.items():
            c = f.code_of(v, lab)
            assert c >= 0, (name, lab)
            w[c] = float(x)
        out.append((v, w))
    return out


def block(per_request):
    """[[(id, weights)]] per request -> the CSR block (l_off, l_vars, v_off, values) of Engine.*(likelihoods=...)."""
    l_off = np.zeros(len(per_request) + 1, np.int64)
    np.cumsum([len(fs) for fs in per_request], out=l_off[1:])
    flat = [x for fs in per_request for x in fs]
    v_off = np.zeros(len(flat) + 1, np.int64)
    np.cumsum([len(w) for _, w in flat], out=v_off[1:])
    values = np.concatenate([np.asarray(w, np.float64) for _, w in flat]) if flat else np.zeros(0)
    return l_off, np.array([v for v, _ in flat], np.int32), v_off, values


# ------------------------------------------------------------------------------------------------------------ the host interpreter
def lh_text(per_request):
    """The --lh file of tools/prog_sim.cpp: per request its number of findings, then variable id and weights (hex) of each."""
    lines = []
    for fs in per_request:
        lines.append(" ".join([str(len(fs))] + [f"{int(v)} " + " ".join(float(x).hex() for x in w) for v, w in fs]))
    return "\n".join(lines) + "\n"


def run_sim(exe, tmp_path, f, kind, requests, per_request=None, options=None, ties=False, dump=False, expect_fail=False):
    """prog_sim `kind` ("max", "map", "ev") over `requests` in the format of the kind's own checker module (mpe_check.net_text,
    map_check.net_text, evidence_check.net_text), with the findings of per_request (None: no --lh at all) -> the CompletedProcess."""
    import evidence_check as ec
    text = {"max": mc.net_text, "map": mp.net_text, "ev": ec.net_text}[kind](f, requests)
    path = os.path.join(str(tmp_path), f"lh_{kind}_net.txt")
    with open(path, "w") as fh:
        fh.write(text)
    cmd = [exe] + (["ev", "run"] if kind == "ev" else [kind]) + [path] + sim_tools.sim_args(f, tmp_path, options, ties)
    if per_request is not None:
        lh = os.path.join(str(tmp_path), f"lh_{kind}.txt")
        with open(lh, "w") as fh:
            fh.write(lh_text(per_request))
        cmd += ["--lh", lh]
    if dump:
        cmd.append("--dump")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if not expect_fail:
        assert r.returncode == 0, r.stderr[-2000:]
    return r


def parse_codes(r):
    """(log_p [B], [codes]) of a max or map run."""
    lp, codes = [], []
    for line in r.stdout.splitlines():
        t = line.split()
        lp.append(-np.inf if t[0] == "-inf" else float.fromhex(t[0]))
        codes.append([int(x) for x in t[1:]])
    return np.array(lp), codes


def parse_tables(r):
    return [np.array([float.fromhex(t) for t in line.split()]) for line in r.stdout.splitlines()]


def parse_dump(r):
    """[(request, arena_cells, seed_cells, program words)] of the lines --dump leaves on standard error."""
    out = []
    for line in r.stderr.splitlines():
        if line.startswith("prog "):
            t = line.split()
            out.append((int(t[1]), int(t[2]), int(t[3]), [int(w, 16) for w in t[4:]]))
    return out
