"""Plain numpy checkers of exact posterior sampling (tests/test_posterior_sampling.py, tests/test_posterior_sampling_host.py): the
dense posterior P(x | e) of a small network, a pooled chi-square test of a sample histogram against it, and the runner of the
host twin tools/prog_sim.cpp draw - all over the flattened network (sorobn_amd.flatten), i.e. the tables the engine itself is given."""
import os
import subprocess

import numpy as np
from scipy.stats import chi2

import mpe_check as mc
import sim_tools

ROOT = mc.ROOT
P_MIN = 1e-6  # false-alarm rate per chi-square check: a few hundred checks fail by chance less than once in a thousand runs


def dense_posterior(f, ev):
    """(variables [k] ascending, P(x | e) as a dense array over them, the unnormalised mass of e) - the product of every CPT,
    evidence sliced, normalised."""
    vs, joint = mc._mul(mc._sliced(f, ev))
    joint = np.asarray(joint, np.float64)
    mass = float(joint.sum())
    return vs, (joint / mass if mass > 0 else joint), mass


def cpts_are_distributions(f):
    """Every CPT row present and summing to 1 within 1e-12 (BayesNet._cpts_are_distributions): pruning is allowed."""
    for v in range(len(f.card)):
        a, b = int(f.value_off[v]), int(f.value_off[v + 1])
        rows = np.asarray(f.values[a:b], np.float64).reshape(-1, int(f.card[v]))
        if not (np.all(np.asarray(f.present[a:b]) == 1.0) and np.all(np.abs(rows.sum(axis=1) - 1.0) <= 1e-12)):
            return False
    return True


def chi_square_p(counts, probs):
    """p-value of Pearson's chi-square of `counts` against expected n * probs.  Cells with an expected count below 5 are pooled
    into one cell; if that pool itself stays below 5 it joins the smallest regular cell.  A count in a cell of probability zero
    gives p = 0.  One cell left after pooling: p = 1."""
    counts = np.asarray(counts, np.float64).reshape(-1)
    probs = np.asarray(probs, np.float64).reshape(-1)
    n = counts.sum()
    if np.any(counts[probs <= 0] > 0):
        return 0.0
    keep = probs > 0
    counts, exp = counts[keep], n * probs[keep]
    small = exp < 5
    obs_c, exp_c = list(counts[~small]), list(exp[~small])
    if small.any():
        obs_c.append(counts[small].sum())
        exp_c.append(exp[small].sum())
        if exp_c[-1] < 5 and len(exp_c) > 1:  # (the pool itself is small: merge it into the smallest regular cell)
            k = int(np.argmin(exp_c[:-1]))
            obs_c[k] += obs_c.pop()
            exp_c[k] += exp_c.pop()
    obs_c, exp_c = np.array(obs_c), np.array(exp_c)
    if len(exp_c) < 2:
        return 1.0
    stat = float(((obs_c - exp_c) ** 2 / exp_c).sum())
    return float(chi2.sf(stat, len(exp_c) - 1))


def histogram(codes, vs, card):
    """Counts of the rows of codes [n, n_vars] over the variables vs, as a dense array of their cardinalities."""
    shape = [int(card[v]) for v in vs]
    if not vs:
        return np.array(float(len(codes)))
    idx = np.ravel_multi_index(tuple(codes[:, v] for v in vs), shape)
    return np.bincount(idx, minlength=int(np.prod(shape))).reshape(shape).astype(np.float64)


def check_samples(f, ev, codes, ctx=""):
    """The acceptance rule of the sampling cases: every row agrees with the evidence and has positive joint probability, and the
    full-state histogram passes the chi-square test against the dense posterior.  Returns the p-value."""
    vs, post, mass = dense_posterior(f, ev)
    assert mass > 0, ctx
    codes = np.asarray(codes)
    for v, c in ev.items():
        assert (codes[:, v] == c).all(), (ctx, "evidence not kept", v)
    assert (codes >= 0).all() and (codes < np.asarray(f.card)[None, :]).all(), (ctx, "code outside its domain")
    h = histogram(codes, vs, f.card)
    assert not np.any(h[post <= 0] > 0), (ctx, "a sample of probability zero")
    p = chi_square_p(h, post)
    assert p >= P_MIN, (ctx, p)
    return p


def sim_text(f, seed, prune, requests):
    """Input of tools/prog_sim.cpp draw: the network, the seed, the prune flag, then the requests [(evars, ecodes, n, g_first)]."""
    parts = sim_tools.network_prefix(f) + [str(int(seed)), str(int(bool(prune))), str(len(requests))]
    for evs, ecs, n, g in requests:
        parts.append(f"{len(evs)} {' '.join(map(str, evs))} {' '.join(map(str, ecs))} {int(n)} {int(g)}")
    return "\n".join(parts) + "\n"


def build_draw_sim(tmp_path):
    return sim_tools.build_prog_sim()


def run_draw_sim(exe, tmp_path, f, seed, prune, requests, margins=False, options=None):
    """(options: None - planned by a bare Network - or the set_option values of the engine whose programs these are, sim_tools.sim_args)
    -> list per request of dict(codes [n, n_vars] int32, p_e, n_steps, n_back, n_fwd, kept_cells, min_margin, low = the global
    rows whose smallest margin is <= 1e-12[, margins [n]]) as tools/prog_sim.cpp draw computes them."""
    d = str(tmp_path)
    path, cpath, mpath = os.path.join(d, "draw_net.txt"), os.path.join(d, "draw_codes.bin"), os.path.join(d, "draw_margins.bin")
    with open(path, "w") as fh:
        fh.write(sim_text(f, seed, prune, requests))
    r = subprocess.run([exe, "draw", path, cpath] + ([mpath] if margins else []) + sim_tools.sim_args(f, tmp_path, options), capture_output=True,
                       text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-2000:]
    nv = len(f.card)
    codes = np.fromfile(cpath, np.int32).reshape(-1, max(1, nv))[:, :nv]
    marg = np.fromfile(mpath, np.float64) if margins else None
    out, row = [], 0
    lines = r.stdout.splitlines()
    assert len(lines) == len(requests), r.stdout[-2000:]
    for (evs, ecs, n, g), line in zip(requests, lines):
        t = line.split()
        k = int(t[6])
        res = dict(codes=codes[row:row + n], p_e=float.fromhex(t[0]), n_steps=int(t[1]), n_back=int(t[2]), n_fwd=int(t[3]),
                   kept_cells=int(t[4]), min_margin=float.fromhex(t[5]), low=[int(x) for x in t[7:7 + k]])
        if margins:
            res["margins"] = marg[row:row + n]
        out.append(res)
        row += n
    assert row == len(codes)
    return out
