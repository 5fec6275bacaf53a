// Host twin of mibn_arc_posteriors' schedule: sorobn_amd/csrc/dag_plan.h (the header dag_post_kernel.hip.h and
// mibn_arc_posteriors include) on a CPU.  It runs the argument check and the centring, then the subset sum by executing the SAME
// pass schedule tile by tile through the body the kernels call (dag_tile_pass over a DagSumTile, with one lane), L and R level by
// level and lane by lane (dag_unrank: lane k takes the k-th subset of the level; dag_level), the superset sum over the same passes
// - the first forming g from L and R while it loads a tile (DagGapTile) -, the candidates' posteriors (dag_log_post) and the arc
// sums in the pinned order (dag_arc_reduce).  A sum's last bits depend on the schedule: under the same options this program
// differs from the device only by the host's exp / log1p.
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
#include <limits>

#include "../sorobn_amd/csrc/dag_plan.h"
#include "sim_io.h"

using namespace mibn;

int main() {
    const SimInput in = read_sim_input();
    const int32_t n = in.n;
    const int64_t n_fam = in.n_fam;
    std::string err;
    if (const int rc = dag_check("arc_posteriors", n, n_fam, in.child.data(), in.parents.data(), in.score.data(), err)) {
        std::printf("{\"error\": %d, \"msg\": \"%s\"}\n", rc, err.c_str());
        return 0;
    }
    const DagPlan D = dag_plan(n, in.tile_bits > 0 ? in.tile_bits : kDagTileBits, in.group_bits > 0 ? in.group_bits : kDagGroupBits);
    std::vector<DagPass> down = D.passes;
    if (down.empty()) down.push_back(DagPass{0, 0, 0});
    const double inf = std::numeric_limits<double>::infinity();
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<double> centre((size_t)n);
    dag_centres(n, n_fam, in.child.data(), in.score.data(), centre.data());
    // fill + scatter
    std::vector<double> alpha((size_t)n * (size_t)D.entries, -inf);
    for (int64_t f = 0; f < n_fam; ++f) {
        const int v = in.child[(size_t)f];
        alpha[(size_t)dag_entry(v, in.parents[(size_t)f], n)] = dag_centred(in.score[(size_t)f], centre[(size_t)v]);
    }
    // the subset sum: pass by pass, workgroup by workgroup (child-major), as dag_post_subset_kernel
    std::vector<double> tile((size_t)1 << kDagMaxTileBits);
    for (const DagPass &P : D.passes) {
        const int64_t per = D.tiles_per_child(P);
        for (int64_t wg = 0; wg < D.grid(P); ++wg) {
            const int64_t v = wg / per, t = wg - v * per;
            dag_tile_pass<true>(DagSumTile{alpha.data(), v << (n - 1), tile.data()}, P, t, 0, 1, DagNoSync{});
        }
    }
    // L and R: level by level, as dag_post_level_kernel
    const size_t subsets = (size_t)1 << n;
    std::vector<double> L(subsets, -inf), R(subsets, -inf);
    const std::vector<uint32_t> binom = dag_binomials();
    for (int level = 0; level <= n; ++level)
        for (uint32_t k = 0; k < binom[(size_t)n * kDagBinomStride + (size_t)level]; ++k) {  // lane k of the level's launch
            const uint32_t S = dag_unrank(k, level, n, binom.data());
            const DagLR x = dag_level(S, n, alpha.data(), L.data(), R.data());
            L[S] = x.l;
            R[S] = x.r;
        }
    // the superset sum into alpha's storage, as dag_post_superset_kernel
    std::vector<double> &gamma = alpha;
    for (size_t k = 0; k < down.size(); ++k) {
        const DagPass &P = down[k];
        const int64_t per = D.tiles_per_child(P);
        for (int64_t wg = 0; wg < D.grid(P); ++wg) {
            const int64_t v = wg / per, t = wg - v * per;
            const DagSumTile T{gamma.data(), v << (n - 1), tile.data()};
            if (k == 0) dag_tile_load(DagGapTile(tile.data(), L.data(), R.data(), (int)v, n), P, P.tile_size(), t, 0, 1);
            else dag_tile_load(T, P, P.tile_size(), t, 0, 1);
            dag_tile_run<false>(T, P, P.tile_size(), t, 0, 1, DagNoSync{});
        }
    }
    // the candidates and the arcs, as dag_post_candidate_kernel, dag_post_arc_kernel and dag_post_arc_sum_kernel
    const double whole = L[subsets - 1];
    std::vector<double> log_post((size_t)n_fam), arc((size_t)n * (size_t)n);
    for (int64_t f = 0; f < n_fam; ++f) {
        const int v = in.child[(size_t)f];
        log_post[(size_t)f] = dag_log_post(v, in.parents[(size_t)f], in.score[(size_t)f], centre[(size_t)v], gamma.data(), whole, n);
    }
    dag_arc_reduce(n, n_fam, in.child.data(), in.parents.data(), log_post.data(), arc.data());
    const std::vector<double> evidence(1, dag_log_evidence(whole, n, centre.data()));
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::printf("{\"schedule\": [");
    for (size_t i = 0; i < D.passes.size(); ++i) std::printf("%s{\"b0\": %d, \"g\": %d, \"c\": %d}", i ? ", " : "", D.passes[i].b0, D.passes[i].g, D.passes[i].c);
    std::printf("]");
    put_bits("log_post_bits", log_post);
    put_bits("arc_bits", arc);
    put_bits("log_evidence_bits", evidence);
    std::printf(", \"seconds\": %.6f", seconds);
    if (in.tables) {
        put_bits("L_bits", L);
        put_bits("R_bits", R);
        put_bits("gamma_bits", gamma);
    }
    std::printf("}\n");
    return 0;
}
