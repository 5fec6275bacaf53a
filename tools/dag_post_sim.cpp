// Host twin of mibn_arc_posteriors' schedule: sorobn_amd/csrc/dag_plan.h (the header dag_post_kernel.hip.h and
// mibn_arc_posteriors include) on a CPU.  It runs the argument check and the centring, then the subset sum by executing the SAME
// pass schedule tile by tile with the same index functions (dag_gather, dag_squeeze, dag_unsqueeze, dag_logaddexp) the kernels
// use, L and R level by level and lane by lane (dag_unrank: lane k takes the k-th subset of the level), the superset sum over the same passes - the first forming g from L and R while it loads a tile -,
// the candidates' posteriors and the arc sums in the pinned order (dag_arc_reduce).  A sum's last bits depend on the schedule:
// under the same options this program differs from the device only by the host's exp / log1p.
//
//   g++ -O2 -std=c++17 -ffp-contract=off tools/dag_post_sim.cpp -o dag_post_sim    (stand-alone: -fsanitize=address,undefined works as it is)
//   dag_post_sim < input
//
// input (white space separated): n_vars tile_bits group_bits tables n_fam, then n_fam triples  child parent_mask score
//   tile_bits / group_bits: the options dag_tile_bits / dag_group_bits, 0 = the default; tables != 0 prints L, R and Gamma too;
//   a score is read by strtod (nan, inf, 0x1p-3 ..)
// output: one JSON object - "schedule" (b0, g, c of every pass of the subset sum), "log_post_bits", "arc_bits" (row = from) and
//   "log_evidence_bits" (the doubles' bits as unsigned integers), "seconds" (everything between the check and the outputs); with
//   tables: "L_bits", "R_bits", "gamma_bits" (child-major) -, or {"error": <MIBN_* code>, "msg": ".."}
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <limits>
#include <string>
#include <vector>

#include "../sorobn_amd/csrc/dag_plan.h"

using namespace mibn;

static long long geti() {
    long long v;
    if (!(std::cin >> v)) { std::fprintf(stderr, "input ends early\n"); std::exit(2); }
    return v;
}
static double getd() {
    std::string tok;
    if (!(std::cin >> tok)) { std::fprintf(stderr, "input ends early\n"); std::exit(2); }
    return std::strtod(tok.c_str(), nullptr);
}
static void put_bits(const char *key, const std::vector<double> &a) {
    std::printf(", \"%s\": [", key);
    for (size_t i = 0; i < a.size(); ++i) {
        unsigned long long u;
        std::memcpy(&u, &a[i], 8);
        std::printf(i ? ", %llu" : "%llu", u);
    }
    std::printf("]");
}

int main() {
    const int32_t n = (int32_t)geti();
    const int tile_bits = (int)geti(), group_bits = (int)geti();
    const bool tables = geti() != 0;
    const int64_t n_fam = geti();
    if (n_fam < 0) { std::fprintf(stderr, "n_fam is negative\n"); return 2; }
    std::vector<int32_t> child((size_t)n_fam);
    std::vector<uint32_t> parents((size_t)n_fam);
    std::vector<double> fam_score((size_t)n_fam);
    for (int64_t f = 0; f < n_fam; ++f) {
        child[(size_t)f] = (int32_t)geti();
        parents[(size_t)f] = (uint32_t)geti();
        fam_score[(size_t)f] = getd();
    }
    std::string err;
    if (const int rc = dag_check(n, n_fam, child.data(), parents.data(), fam_score.data(), err)) {
        std::printf("{\"error\": %d, \"msg\": \"%s\"}\n", rc, err.c_str());
        return 0;
    }
    const DagPlan D = dag_plan(n, tile_bits > 0 ? tile_bits : kDagTileBits, group_bits > 0 ? group_bits : kDagGroupBits);
    std::vector<DagPass> down = D.passes;
    if (down.empty()) down.push_back(DagPass{0, 0, 0});
    const double inf = std::numeric_limits<double>::infinity();
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<double> centre((size_t)n);
    dag_centres(n, n_fam, child.data(), fam_score.data(), centre.data());
    // fill + scatter
    std::vector<double> alpha((size_t)n * (size_t)D.entries, -inf);
    for (int64_t f = 0; f < n_fam; ++f) {
        const int v = child[(size_t)f];
        alpha[(size_t)(((int64_t)v << (n - 1)) + dag_squeeze(parents[(size_t)f], v))] = dag_centred(fam_score[(size_t)f], centre[(size_t)v]);
    }
    // the subset sum: pass by pass, workgroup by workgroup (child-major), as dag_post_subset_kernel
    std::vector<double> tile((size_t)1 << kDagMaxTileBits);
    for (const DagPass &P : D.passes) {
        const int64_t per = D.tiles_per_child(P), size = P.tile_entries();
        for (int64_t wg = 0; wg < D.grid(P); ++wg) {
            const int64_t v = wg / per, t = wg - v * per, base = v << (n - 1);
            for (int64_t e = 0; e < size; ++e) tile[(size_t)e] = alpha[(size_t)(base + dag_gather(P, t, e))];
            for (int b = P.c; b < P.c + P.g; ++b) {
                const int64_t low = (int64_t(1) << b) - 1;
                for (int64_t p = 0; p < size / 2; ++p) {
                    const size_t e0 = (size_t)((p & low) | ((p & ~low) << 1)), e1 = e0 | ((size_t)1 << b);
                    tile[e1] = dag_logaddexp(tile[e1], tile[e0]);
                }
            }
            for (int64_t e = 0; e < size; ++e) alpha[(size_t)(base + dag_gather(P, t, e))] = tile[(size_t)e];
        }
    }
    // L and R: level by level, as dag_post_level_kernel
    const size_t subsets = (size_t)1 << n;
    const uint32_t full = (uint32_t)(subsets - 1);
    std::vector<double> L(subsets, -inf), R(subsets, -inf);
    std::vector<uint32_t> binom((size_t)kDagBinomStride * kDagBinomStride);
    dag_binomials(binom.data());
    for (int level = 0; level <= n; ++level)
        for (uint32_t k = 0; k < binom[(size_t)n * kDagBinomStride + (size_t)level]; ++k) {  // lane k of the level's launch
            const uint32_t S = dag_unrank(k, level, n, binom.data());
            const size_t S64 = S;
            const uint32_t outside = full ^ S;
            double l = S ? -inf : 0.0, r = l;
            for (uint32_t rest = S; rest; rest &= rest - 1) {
                const int v = __builtin_ctz(rest);
                const uint32_t C = S ^ (1u << v);
                const int64_t base = (int64_t)v << (n - 1);
                l = dag_logaddexp(l, L[C] + alpha[(size_t)(base + dag_squeeze(C, v))]);
                r = dag_logaddexp(r, alpha[(size_t)(base + dag_squeeze(outside, v))] + R[C]);
            }
            L[S64] = l;
            R[S64] = r;
        }
    // the superset sum into alpha's storage, as dag_post_superset_kernel
    std::vector<double> &gamma = alpha;
    for (size_t k = 0; k < down.size(); ++k) {
        const DagPass &P = down[k];
        const int64_t per = D.tiles_per_child(P), size = P.tile_entries();
        for (int64_t wg = 0; wg < D.grid(P); ++wg) {
            const int64_t v = wg / per, t = wg - v * per, base = v << (n - 1);
            const uint32_t others = full ^ (1u << (int)v);
            for (int64_t e = 0; e < size; ++e) {
                if (k == 0) {
                    const uint32_t S = dag_unsqueeze((uint32_t)dag_gather(P, t, e), (int)v);
                    tile[(size_t)e] = L[S] + R[others ^ S];
                } else {
                    tile[(size_t)e] = gamma[(size_t)(base + dag_gather(P, t, e))];
                }
            }
            for (int b = P.c; b < P.c + P.g; ++b) {
                const int64_t low = (int64_t(1) << b) - 1;
                for (int64_t p = 0; p < size / 2; ++p) {
                    const size_t e0 = (size_t)((p & low) | ((p & ~low) << 1)), e1 = e0 | ((size_t)1 << b);
                    tile[e0] = dag_logaddexp(tile[e0], tile[e1]);
                }
            }
            for (int64_t e = 0; e < size; ++e) gamma[(size_t)(base + dag_gather(P, t, e))] = tile[(size_t)e];
        }
    }
    // the candidates and the arcs, as dag_post_candidate_kernel, dag_post_arc_kernel and dag_post_arc_sum_kernel
    const double whole = L[full];
    std::vector<double> log_post((size_t)n_fam), arc((size_t)n * (size_t)n);
    for (int64_t f = 0; f < n_fam; ++f) {
        const int v = child[(size_t)f];
        const double s = dag_centred(fam_score[(size_t)f], centre[(size_t)v]);
        const double g = gamma[(size_t)(((int64_t)v << (n - 1)) + dag_squeeze(parents[(size_t)f], v))];
        log_post[(size_t)f] = whole == -inf ? whole : (s + g) - whole;
    }
    dag_arc_reduce(n, n_fam, child.data(), parents.data(), log_post.data(), arc.data());
    const std::vector<double> evidence(1, dag_log_evidence(whole, n, centre.data()));
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::printf("{\"schedule\": [");
    for (size_t i = 0; i < D.passes.size(); ++i) std::printf("%s{\"b0\": %d, \"g\": %d, \"c\": %d}", i ? ", " : "", D.passes[i].b0, D.passes[i].g, D.passes[i].c);
    std::printf("]");
    put_bits("log_post_bits", log_post);
    put_bits("arc_bits", arc);
    put_bits("log_evidence_bits", evidence);
    std::printf(", \"seconds\": %.6f", seconds);
    if (tables) {
        put_bits("L_bits", L);
        put_bits("R_bits", R);
        put_bits("gamma_bits", gamma);
    }
    std::printf("}\n");
    return 0;
}
