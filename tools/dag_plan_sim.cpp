// Host twin of mibn_best_dag's schedule: sorobn_amd/csrc/dag_plan.h (the header dag_kernel.hip.h and mibn_best_dag include) on a
// CPU.  It runs the argument check, then phase A by executing the SAME pass schedule tile by tile with the same index functions
// (dag_gather, dag_squeeze, dag_better) the kernels use, then phase B level by level and the traceback - the index arithmetic of
// gathered tiles and ragged groups under a CPU test, and a CPU yardstick for tools/bench_exact.py.
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
static unsigned long long bits_of(double x) {
    unsigned long long u;
    std::memcpy(&u, &x, 8);
    return u;
}
template <class T, class F>
static void put_list(const char *key, const std::vector<T> &a, F &&item) {
    std::printf(", \"%s\": [", key);
    for (size_t i = 0; i < a.size(); ++i) std::printf(i ? ", %llu" : "%llu", (unsigned long long)item(a[i]));
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
    const double inf = std::numeric_limits<double>::infinity();
    const auto t0 = std::chrono::steady_clock::now();
    // fill + scatter
    std::vector<double> score((size_t)n * (size_t)D.entries, -inf);
    std::vector<uint32_t> mask(score.size(), kDagNoMask);
    for (int64_t f = 0; f < n_fam; ++f) {
        const int v = child[(size_t)f];
        const size_t at = (size_t)(((int64_t)v << (n - 1)) + dag_squeeze(parents[(size_t)f], v));
        score[at] = fam_score[(size_t)f];
        mask[at] = parents[(size_t)f];
    }
    // phase A: pass by pass, workgroup by workgroup (child-major), as dag_subset_kernel
    std::vector<double> s_score((size_t)1 << kDagMaxTileBits);
    std::vector<uint32_t> s_mask(s_score.size());
    for (const DagPass &P : D.passes) {
        const int64_t per = D.tiles_per_child(P), size = P.tile_entries();
        for (int64_t wg = 0; wg < D.grid(P); ++wg) {
            const int64_t v = wg / per, t = wg - v * per, base = v << (n - 1);
            for (int64_t e = 0; e < size; ++e) {
                const size_t at = (size_t)(base + dag_gather(P, t, e));
                s_score[(size_t)e] = score[at];
                s_mask[(size_t)e] = mask[at];
            }
            for (int b = P.c; b < P.c + P.g; ++b) {
                const int64_t low = (int64_t(1) << b) - 1;
                for (int64_t p = 0; p < size / 2; ++p) {
                    const size_t e0 = (size_t)((p & low) | ((p & ~low) << 1)), e1 = e0 | ((size_t)1 << b);
                    if (dag_better(s_score[e0], s_mask[e0], s_score[e1], s_mask[e1])) {
                        s_score[e1] = s_score[e0];
                        s_mask[e1] = s_mask[e0];
                    }
                }
            }
            for (int64_t e = 0; e < size; ++e) {
                const size_t at = (size_t)(base + dag_gather(P, t, e));
                score[at] = s_score[(size_t)e];
                mask[at] = s_mask[(size_t)e];
            }
        }
    }
    // phase B: level by level, as dag_sink_kernel
    const size_t subsets = (size_t)1 << n;
    std::vector<double> best(subsets, -inf);
    std::vector<uint8_t> sink(subsets, (uint8_t)kDagNoSink);
    for (int level = 0; level <= n; ++level)
        for (size_t S64 = 0; S64 < subsets; ++S64) {
            const uint32_t S = (uint32_t)S64;
            if (__builtin_popcount(S) != level) continue;
            double top = S ? -inf : 0.0;
            int who = kDagNoSink;
            for (uint32_t rest = S; rest; rest &= rest - 1) {
                const int v = __builtin_ctz(rest);
                const uint32_t C = S ^ (1u << v);
                const double term = best[C] + score[(size_t)(((int64_t)v << (n - 1)) + dag_squeeze(C, v))];
                if (term > top) { top = term; who = v; }
            }
            best[S64] = top;
            sink[S64] = (uint8_t)who;
        }
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    // traceback, as dag_traceback_kernel
    std::vector<uint32_t> parents_out((size_t)n, kDagNoMask);
    std::vector<int32_t> order_out((size_t)n, -1);
    uint32_t S = (uint32_t)(subsets - 1);
    const double total = best[S];
    if (sink[S] != kDagNoSink)
        for (int k = n - 1; k >= 0; --k) {
            const int v = sink[S];
            S ^= 1u << v;
            parents_out[(size_t)v] = mask[(size_t)(((int64_t)v << (n - 1)) + dag_squeeze(S, v))];
            order_out[(size_t)k] = v;
        }
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
    if (tables) {
        put_list("bps_score_bits", score, bits_of);
        put_list("bps_mask", mask, [](uint32_t x) { return x; });
        put_list("best_bits", best, bits_of);
        put_list("sink", sink, [](uint8_t x) { return x; });
    }
    std::printf("}\n");
    return 0;
}
