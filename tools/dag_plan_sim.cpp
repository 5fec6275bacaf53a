// Host twin of mibn_best_dag's schedule: sorobn_amd/csrc/dag_plan.h (the header dag_kernel.hip.h and mibn_best_dag include) on a
// CPU.  It runs the argument check, then phase A by executing the SAME pass schedule tile by tile through the body the kernel calls
// (dag_tile_pass over a DagMaxTile, with one lane), then phase B level by level (dag_sink) and the traceback (dag_traceback) - the
// index arithmetic of gathered tiles and ragged groups under a CPU test, and a CPU yardstick for tools/bench_exact.py.
//
//   g++ -O2 -std=c++17 tools/dag_plan_sim.cpp -o dag_plan_sim         (stand-alone: -fsanitize=address,undefined works as it is)
//   dag_plan_sim < input
//
// input (white space separated): n_vars tile_bits group_bits tables n_fam, then n_fam triples  child parent_mask score
//   tile_bits / group_bits: the options dag_tile_bits / dag_group_bits, 0 = the default; tables != 0 prints the four tables too;
//   a score is read by strtod (nan, inf, 0x1p-3 ..)
// output: one JSON object - "schedule" (b0, g, c, tiles_per_child, grid of every pass), "parents", "order", "total" (%.17g; -inf
//   as the string "-inf") and "total_bits" (the double's bits as an unsigned integer), "seconds" (phases A and B); with tables:
//   "bps_score_bits", "bps_mask" (child-major), "best_bits", "sink" -, or {"error": <MIBN_* code>, "msg": ".."}
#include <chrono>
#include <limits>

#include "../sorobn_amd/csrc/dag_plan.h"
#include "sim_io.h"

using namespace mibn;

int main() {
    const SimInput in = read_sim_input();
    const int32_t n = in.n;
    std::string err;
    if (const int rc = dag_check("best_dag", n, in.n_fam, in.child.data(), in.parents.data(), in.score.data(), err)) {
        std::printf("{\"error\": %d, \"msg\": \"%s\"}\n", rc, err.c_str());
        return 0;
    }
    const DagPlan D = dag_plan(n, in.tile_bits > 0 ? in.tile_bits : kDagTileBits, in.group_bits > 0 ? in.group_bits : kDagGroupBits);
    const double inf = std::numeric_limits<double>::infinity();
    const auto t0 = std::chrono::steady_clock::now();
    // fill + scatter
    std::vector<double> score((size_t)n * (size_t)D.entries, -inf);
    std::vector<uint32_t> mask(score.size(), kDagNoMask);
    for (int64_t f = 0; f < in.n_fam; ++f) {
        const size_t at = (size_t)dag_entry(in.child[(size_t)f], in.parents[(size_t)f], n);
        score[at] = in.score[(size_t)f];
        mask[at] = in.parents[(size_t)f];
    }
    // phase A: pass by pass, workgroup by workgroup (child-major), as dag_subset_kernel
    std::vector<double> s_score((size_t)1 << kDagMaxTileBits);
    std::vector<uint32_t> s_mask(s_score.size());
    for (const DagPass &P : D.passes) {
        const int64_t per = D.tiles_per_child(P);
        for (int64_t wg = 0; wg < D.grid(P); ++wg) {
            const int64_t v = wg / per, t = wg - v * per;
            dag_tile_pass<true>(DagMaxTile{score.data(), mask.data(), v << (n - 1), s_score.data(), s_mask.data()}, P, t, 0, 1, DagNoSync{});
        }
    }
    // phase B: level by level, as dag_sink_kernel
    const size_t subsets = (size_t)1 << n;
    std::vector<double> best(subsets, -inf);
    std::vector<uint8_t> sink(subsets, (uint8_t)kDagNoSink);
    for (int level = 0; level <= n; ++level)
        for (size_t S = 0; S < subsets; ++S) {
            if (__builtin_popcount((uint32_t)S) != level) continue;
            const DagSink r = dag_sink((uint32_t)S, n, score.data(), best.data());
            best[S] = r.top;
            sink[S] = (uint8_t)r.who;
        }
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    // the traceback, as dag_traceback_kernel
    std::vector<uint32_t> parents_out((size_t)n);
    std::vector<int32_t> order_out((size_t)n);
    double total;
    dag_traceback(mask.data(), best.data(), sink.data(), n, parents_out.data(), order_out.data(), &total);
    std::printf("{\"schedule\": [");
    for (size_t i = 0; i < D.passes.size(); ++i) {
        const DagPass &P = D.passes[i];
        std::printf("%s{\"b0\": %d, \"g\": %d, \"c\": %d, \"tiles_per_child\": %lld, \"grid\": %lld}", i ? ", " : "", P.b0, P.g, P.c,
                    (long long)D.tiles_per_child(P), (long long)D.grid(P));
    }
    std::printf("]");
    put_list("parents", parents_out, [](uint32_t x) { return x; });
    std::printf(", \"order\": [");
    for (size_t i = 0; i < order_out.size(); ++i) std::printf(i ? ", %d" : "%d", order_out[i]);
    std::printf("]");
    if (total == -inf) std::printf(", \"total\": \"-inf\"");
    else std::printf(", \"total\": %.17g", total);
    std::printf(", \"total_bits\": %llu, \"seconds\": %.6f", bits_of(total), seconds);
    if (in.tables) {
        put_list("bps_score_bits", score, bits_of);
        put_list("bps_mask", mask, [](uint32_t x) { return x; });
        put_list("best_bits", best, bits_of);
        put_list("sink", sink, [](uint8_t x) { return x; });
    }
    std::printf("}\n");
    return 0;
}
