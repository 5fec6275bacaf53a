// Host interpreter of draw programs (planner.h, "DRAW programs") and of their draw records: the CPU twin of
// mibn_posterior_sample_batch - same programs, same Philox4x32-10 stream, same arithmetic of the draw - independent of the
// kernels (tests/test_posterior_sampling_host.py builds and runs it; tests/test_posterior_sampling.py compares the device with it).
//
//   g++ -O2 -mpopcnt -std=c++17 -ffp-contract=off tools/draw_sim.cpp sorobn_amd/csrc/planner.cpp -lpthread -o draw_sim
//   ./draw_sim net.txt codes.bin [margins.bin]
//
// Input (whitespace-separated): n_vars, card[n], scope_off[n + 1], scope_vars[], value_off[n + 1], values[] (any strtod
// format), seed, prune (0 / 1), B, then per request: ne, evars[ne], ecodes[ne], n_samples, g_first (the global row index of its
// first sample: the Philox counter).  codes.bin receives the rows of all requests, int32[n_vars] each, in request order;
// margins.bin (optional) one double per row: the smallest margin of its draws, min_x |u * total - acc_x| / total - how far the
// nearest boundary of the running sum was from the uniform.  Standard output, one line per request:
//   p_e (%a)  n_steps  n_back  n_fwd  kept_cells  smallest margin (%a)  k  g_1 .. g_k     (the k rows whose margin is <= 1e-12)
// Besides running the programs it checks, and exits 1 with a message when one fails:
//   * every step is GENERIC, none carries the MAX flag, the FINAL step is one cell and carries the RAW flag;
//   * no table of a request overlaps another one (nothing is released: every intermediate lives until the draw), every arena
//     access lies inside the request's arena_cells, and PlanStats::kept_cells accounts for all of them;
//   * the record has one backward entry per elimination step, and every variable a draw reads is evidence or drawn before;
//   * a draw never meets a zero total when the mass is positive.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "sim_common.h"

using namespace mibn;

// Philox4x32-10, counter = (i lo, i hi, stream, 0): gibbs_kernel.hip.h, philox_uniform
static double philox_uniform(uint64_t i, uint32_t stream, uint32_t k0, uint32_t k1) {
    uint32_t c[4] = {(uint32_t)i, (uint32_t)(i >> 32), stream, 0u};
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    const uint64_t m = ((uint64_t)c[0] << 21) ^ (uint64_t)(c[1] >> 11);
    return (double)(m & ((1ull << 53) - 1)) * (1.0 / 9007199254740992.0);
}

int main(int argc, char **argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: draw_sim net.txt codes.bin [margins.bin]\n"); return 2; }
    slurp(argv[1]);
    FILE *fc = std::fopen(argv[2], "wb");
    if (!fc) { std::perror(argv[2]); return 2; }
    FILE *fm = argc > 3 ? std::fopen(argv[3], "wb") : nullptr;
    if (argc > 3 && !fm) { std::perror(argv[3]); return 2; }
    Network net;
    read_network(net);
    const int n = net.n_vars;
    const std::vector<int32_t> &card = net.card;
    const uint64_t seed = getu();
    const bool prune = geti() != 0;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32) ^ 0x85EBCA6Bu;  // (the key of mibn_sample)
    const int64_t B = geti();
    for (int64_t b = 0; b < B; ++b) {
        const int ne = (int)geti();
        std::vector<int32_t> ev(ne), ec(ne);
        for (auto &v : ev) v = (int32_t)geti();
        for (auto &c : ec) c = (int32_t)geti();
        const int64_t n_samples = geti();
        const uint64_t g_first = getu();
        std::vector<int32_t> row(n);
        auto write_none = [&]() {  // zero mass: -1 for every non-evidence variable
            for (int v = 0; v < n; ++v) row[v] = -1;
            for (int i = 0; i < ne; ++i) row[ev[i]] = ec[i];
            const double one = 1.0;
            for (int64_t s = 0; s < n_samples; ++s) {
                std::fwrite(row.data(), 4, (size_t)n, fc);
                if (fm) std::fwrite(&one, 8, 1, fm);
            }
        };
        bool out_of_domain = false;
        for (int i = 0; i < ne; ++i) out_of_domain = out_of_domain || ec[i] < 0 || ec[i] >= card[ev[i]];
        if (out_of_domain) {  // (the engine skips such a request: zero probability)
            write_none();
            std::printf("%a 0 0 0 0 %a 0\n", 0.0, 1.0);
            continue;
        }
        Request rq;
        rq.ne = ne;
        rq.evars = ev.data();
        rq.ecodes = ec.data();
        rq.kind = ProgramKind::Draw;
        rq.no_prune = !prune;
        const std::string ve = validate_mpe_request(net, rq);
        if (!ve.empty()) fail(b, ve);
        std::vector<uint32_t> prog;
        PlanStats st;
        const std::string pe = plan_request(net, rq, prog, st);
        if (!pe.empty()) fail(b, pe);
        if (st.kept_cells != st.arena_cells) fail(b, "kept_cells " + std::to_string(st.kept_cells) + " != arena_cells " + std::to_string(st.arena_cells));
        std::vector<double> arena((size_t)std::max<int64_t>(16, st.arena_cells), std::nan(""));
        auto arena_at = [&](int64_t i) -> double & {
            if (i < 0 || i >= (int64_t)arena.size()) fail(b, "arena access " + std::to_string(i) + " outside " + std::to_string(arena.size()) + " cells");
            return arena[(size_t)i];
        };
        const uint32_t n_steps = prog[0];
        double mass = n_steps ? 0.0 : 1.0;  // (no step at all: the empty product)
        std::vector<std::pair<int64_t, int64_t>> tabs;
        size_t off = 1;
        int n_elim = 0;
        bool seen_final = false;
        for (uint32_t s = 0; s < n_steps; ++s) {
            const GenericStep g(b, s, prog.data() + off);
            const int cx = g.cx;
            const uint32_t flags = g.flags;
            const bool fin = flags & kFlagFinal;
            if (flags & kFlagMax) fail(b, "step " + std::to_string(s) + " carries the MAX flag");
            if (fin != (s + 1 == n_steps)) fail(b, "the FINAL step is not the last one");
            if (fin && !(flags & kFlagRaw)) fail(b, "FINAL step without the RAW flag");
            if (fin && cx > 1) fail(b, "FINAL step eliminates a variable");
            if (cx > 1) ++n_elim;
            const int64_t cells = g.cells, out_off = g.out_off;
            if (!fin) {
                for (auto &t : tabs)
                    if (out_off < t.first + t.second && t.first < out_off + cells) fail(b, "the output of step " + std::to_string(s) + " overlaps a kept table");
                tabs.push_back({out_off, cells});
            }
            std::vector<double> outv((size_t)cells, 0.0);
            g.visit(net, arena_at, [&](int64_t o, int, double prod) { outv[(size_t)o] += prod; });  // sum over x
            if (fin) {
                if (cells != 1 || out_off != 0) fail(b, "FINAL step of more than one cell");
                mass = outv[0];
                seen_final = true;
            } else {
                for (int64_t o = 0; o < cells; ++o) arena_at(out_off + o) = outv[(size_t)o];
            }
            off += g.words;
        }
        if (n_steps && !seen_final) fail(b, "no FINAL step");
        // the record
        const uint32_t *rec = prog.data() + off;
        const uint32_t n_back = rec[0], n_fwd = rec[1], n_ev = rec[2];
        if ((int)n_back != n_elim) fail(b, "draw record has " + std::to_string(n_back) + " backward entries for " + std::to_string(n_elim) + " elimination steps");
        if ((int)n_ev != ne) fail(b, "draw record names " + std::to_string(n_ev) + " evidence variables");
        rec += 3;
        std::vector<char> known0(n, 0);
        for (int v = 0; v < n; ++v) known0[v] = card[v] <= 1;
        for (uint32_t i = 0; i < n_ev; ++i) known0[rec[2 * i]] = 1;
        const uint32_t *ev_rec = rec;
        rec += 2 * n_ev;
        {   // every variable a draw reads is evidence or drawn before; every variable ends up drawn
            std::vector<char> known = known0;
            const uint32_t *r2 = rec;
            for (uint32_t i = 0; i < n_back + n_fwd; ++i) {
                const int x = (int)r2[0];
                const uint32_t n_in = r2[2];
                if ((int)r2[1] != card[x]) fail(b, "draw entry with a wrong cardinality");
                if (known[x]) fail(b, "variable " + std::to_string(x) + " is drawn twice (or is evidence)");
                if (i >= n_back && n_in != 1) fail(b, "forward entry with more than one input");
                r2 += 3;
                for (uint32_t j = 0; j < n_in; ++j) {
                    const uint32_t n_ax = r2[3];
                    for (uint32_t a = 0; a < n_ax; ++a)
                        if (!known[r2[4 + 2 * a]]) fail(b, "the draw of " + std::to_string(x) + " reads variable " + std::to_string(r2[4 + 2 * a]) + " before it is drawn");
                    r2 += 4 + 2 * n_ax;
                }
                known[x] = 1;
            }
            for (int v = 0; v < n; ++v)
                if (!known[v]) fail(b, "variable " + std::to_string(v) + " is never drawn");
        }
        if (!(mass > 0)) {
            write_none();
            std::printf("%a %u %u %u %lld %a 0\n", 0.0, n_steps, n_back, n_fwd, (long long)st.kept_cells, 1.0);
            continue;
        }
        double min_margin = 1.0;
        std::vector<uint64_t> low;
        std::vector<double> wv;
        for (int64_t s = 0; s < n_samples; ++s) {
            const uint64_t g = g_first + (uint64_t)s;
            for (int v = 0; v < n; ++v) row[v] = 0;
            for (uint32_t i = 0; i < n_ev; ++i) row[ev_rec[2 * i]] = (int32_t)ev_rec[2 * i + 1];
            const uint32_t *r2 = rec;
            double row_margin = 1.0;
            for (uint32_t i = 0; i < n_back + n_fwd; ++i) {
                const int x = (int)r2[0], cx = (int)r2[1];
                const uint32_t n_in = r2[2];
                r2 += 3;
                wv.assign((size_t)cx, 0.0);
                for (uint32_t j = 0; j < n_in; ++j) {
                    const uint64_t in_off = (uint64_t)r2[0] | ((uint64_t)r2[1] << 32);
                    const int64_t xs = (int64_t)r2[2];
                    const uint32_t n_ax = r2[3];
                    int64_t idx = 0;
                    for (uint32_t a = 0; a < n_ax; ++a) idx += (int64_t)row[r2[4 + 2 * a]] * (int64_t)r2[5 + 2 * a];
                    for (int c = 0; c < cx; ++c) {
                        const int64_t ii = idx + c * xs;
                        const double p = (in_off & kConstFlag) ? net.pool[(size_t)((in_off & ~kConstFlag) + ii)] : arena_at((int64_t)in_off + ii);
                        wv[(size_t)c] = j ? wv[(size_t)c] * p : p;
                    }
                    r2 += 4 + 2 * n_ax;
                }
                double total = 0;
                for (int c = 0; c < cx; ++c) total += wv[(size_t)c];
                if (!(total > 0)) fail(b, "the draw of variable " + std::to_string(x) + " meets a zero total at positive mass");
                const double u = philox_uniform(g, 2u + (uint32_t)x, k0, k1) * total;
                double acc = 0;
                int val = -1, last_pos = 0;
                for (int c = 0; c < cx; ++c) {
                    acc += wv[(size_t)c];
                    if (wv[(size_t)c] > 0) last_pos = c;
                    if (val < 0 && u < acc) val = c;
                    row_margin = std::min(row_margin, std::fabs(u - acc) / total);
                }
                if (val < 0) val = last_pos;  // (rounding: the last state of positive weight, never a zero-weight one)
                row[x] = val;
            }
            std::fwrite(row.data(), 4, (size_t)n, fc);
            if (fm) std::fwrite(&row_margin, 8, 1, fm);
            min_margin = std::min(min_margin, row_margin);
            if (row_margin <= 1e-12) low.push_back(g);
        }
        std::printf("%a %u %u %u %lld %a %zu", mass, n_steps, n_back, n_fwd, (long long)st.kept_cells, min_margin, low.size());
        for (uint64_t g : low) std::printf(" %llu", (unsigned long long)g);
        std::printf("\n");
    }
    std::fclose(fc);
    if (fm) std::fclose(fm);
    return 0;
}
