// Host interpreter of map programs (planner.h, "MAP programs"), of their traceback records and gather lists: pins the emission of
// mibn_map_batch independently of the kernels (tests/test_map_host.py builds and runs it).
//
//   g++ -O2 -mpopcnt -std=c++17 tools/map_sim.cpp sorobn_amd/csrc/planner.cpp -lpthread -o map_sim && ./map_sim net.txt
//
// Input (whitespace-separated): n_vars, card[n], scope_off[n + 1], scope_vars[], value_off[n + 1], values[] (any strtod
// format), B, then per request: no_prune (0 / 1), nm, mvars[nm], ne, evars[ne], ecodes[ne].  Output: one line per request,
// "log_p code_0 .. code_{nm-1}" (log_p as %a, or -inf; the codes of mvars in the order given).  It runs the program as written -
// a flagged step maximises, any other step sums - and checks, exiting 1 with a message when one fails:
//   * every step is GENERIC;
//   * no unflagged step eliminates a variable (cx > 1) after the first MAX step; no product-only step carries the flag;
//   * the record has one entry per MAX step, and every MAX step eliminates a variable of M (the entry's variable, of the step's cx);
//   * the argmax tables of a request overlap neither each other nor an intermediate while it is live;
//   * every axis of a traceback entry is a MAP variable decoded before it is used;
//   * the gather list is M in the caller's order; every arena access lies inside the request's arena_cells.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "sim_common.h"

using namespace mibn;

int main(int argc, char **argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: map_sim net.txt\n"); return 2; }
    slurp(argv[1]);
    Network net;
    read_network(net);
    const int n = net.n_vars;
    const std::vector<int32_t> &card = net.card;
    const int64_t B = geti();
    for (int64_t b = 0; b < B; ++b) {
        const bool no_prune = geti() != 0;
        const int nm = (int)geti();
        std::vector<int32_t> mv(nm);
        for (auto &v : mv) v = (int32_t)geti();
        const int ne = (int)geti();
        std::vector<int32_t> ev(ne), ec(ne);
        for (auto &v : ev) v = (int32_t)geti();
        for (auto &c : ec) c = (int32_t)geti();
        bool out_of_domain = false;
        for (int i = 0; i < ne; ++i) out_of_domain = out_of_domain || ec[i] < 0 || ec[i] >= card[ev[i]];
        auto print_zero = [&] {
            std::printf("-inf");
            for (int k = 0; k < nm; ++k) std::printf(" -1");
            std::printf("\n");
        };
        Request rq;
        rq.nq = nm;
        rq.qvars = mv.data();
        rq.ne = ne;
        rq.evars = ev.data();
        rq.ecodes = ec.data();
        rq.kind = ProgramKind::Map;
        rq.no_prune = no_prune;
        const std::string ve = validate_request(net, rq);
        if (!ve.empty()) fail(b, ve);
        if (out_of_domain) { print_zero(); continue; }  // (the engine skips such a request: zero probability)
        std::vector<uint32_t> prog;
        PlanStats st;
        const std::string pe = plan_request(net, rq, prog, st);
        if (!pe.empty()) fail(b, pe);
        std::vector<char> in_m(n, 0);
        for (int32_t v : mv) in_m[v] = 1;
        std::vector<double> arena((size_t)std::max<int64_t>(16, st.arena_cells), std::nan(""));
        const uint32_t n_steps = prog[0];
        double m = n_steps ? 0.0 : 1.0;  // (no step at all: the empty product, written by the host)
        struct Table { int64_t off, cells; int written, last_read; };
        std::vector<Table> tabs;                      // intermediates
        std::vector<std::pair<int64_t, int64_t>> am;  // argmax regions (doubles)
        std::vector<int> am_step, am_cx;
        auto arena_at = [&](int64_t i) -> double & {
            if (i < 0 || i >= (int64_t)arena.size()) fail(b, "arena access " + std::to_string(i) + " outside " + std::to_string(arena.size()) + " cells");
            return arena[(size_t)i];
        };
        size_t off = 1;
        bool max_phase = false, saw_final = false;
        for (uint32_t s = 0; s < n_steps; ++s) {
            const GenericStep g(b, s, prog.data() + off);
            const int n_in = g.n_in, cx = g.cx;
            const bool fin = g.flags & kFlagFinal, mx = g.flags & kFlagMax;
            if (cx <= 1 && mx) fail(b, "product step " + std::to_string(s) + " with the MAX flag");
            if (cx > 1 && !mx && max_phase) fail(b, "sum step " + std::to_string(s) + " after the first MAX step");
            if (fin && (s + 1 != n_steps || !(g.flags & kFlagRaw) || cx > 1)) fail(b, "FINAL step " + std::to_string(s) + " is not the last, not RAW or eliminates");
            max_phase = max_phase || mx;
            saw_final = saw_final || fin;
            const int64_t cells = g.cells, out_off = g.out_off;
            for (int j = 0; j < n_in; ++j)
                if (!(g.in_off[j] & kConstFlag))
                    for (size_t t = tabs.size(); t-- > 0;)
                        if (tabs[t].off == (int64_t)g.in_off[j]) { tabs[t].last_read = (int)s; break; }
            if (mx) {
                const int64_t am_cells = (cells * 2 + 7) / 8;
                for (auto &r : am)
                    if (g.am_off < r.first + r.second && r.first < g.am_off + am_cells) fail(b, "argmax tables overlap");
                am.push_back({g.am_off, am_cells});
                am_step.push_back((int)s);
                am_cx.push_back(cx);
                arena_at(g.am_off + am_cells - 1);
            }
            if (!fin) tabs.push_back({out_off, cells, (int)s, (int)s});
            std::vector<double> outv((size_t)cells);
            std::vector<uint16_t> arg((size_t)cells);
            g.visit(net, arena_at, [&](int64_t o, int x, double prod) {
                if (mx) {  // max over x, the lowest x that attains it
                    if (x == 0 || prod > outv[(size_t)o]) { outv[(size_t)o] = prod; arg[(size_t)o] = (uint16_t)x; }
                } else {   // the sum body: 0.0 + the terms in ascending x
                    outv[(size_t)o] = (x == 0 ? 0.0 : outv[(size_t)o]) + prod;
                }
            });
            if (fin) {
                if (cells != 1 || out_off != 0) fail(b, "FINAL step of more than one cell");
                m = outv[0];
            } else {
                for (int64_t o = 0; o < cells; ++o) arena_at(out_off + o) = outv[(size_t)o];
            }
            if (mx) std::memcpy(reinterpret_cast<char *>(arena.data() + g.am_off), arg.data(), (size_t)cells * 2);
            off += g.words;
        }
        if (n_steps && !saw_final) fail(b, "no FINAL step");
        // a table written at step s and last read at step t is live over [s, t]: the argmax table of step k must not overlap it when
        // s <= k <= t, nor may a later intermediate overwrite an argmax table
        for (size_t a = 0; a < am.size(); ++a)
            for (const Table &t : tabs) {
                const bool overlap = am[a].first < t.off + t.cells && t.off < am[a].first + am[a].second;
                if (overlap && (t.written >= am_step[a] || t.last_read >= am_step[a]))
                    fail(b, "argmax table of step " + std::to_string(am_step[a]) + " overlaps a live intermediate");
            }
        // traceback record
        const uint32_t *rec = prog.data() + off;
        const uint32_t n_rec = rec[0], n_ev = rec[1];
        if (n_rec != am.size()) fail(b, "traceback record has " + std::to_string(n_rec) + " entries for " + std::to_string(am.size()) + " MAX steps");
        if ((int)n_ev != ne) fail(b, "traceback record names " + std::to_string(n_ev) + " evidence variables");
        rec += 2 + 2 * n_ev;
        std::vector<int32_t> code(n, 0);
        std::vector<char> known(n, 0);
        for (int v = 0; v < n; ++v) known[v] = in_m[v] && card[v] <= 1;  // (a single-state MAP variable is never eliminated: code 0)
        for (uint32_t i = 0; i < n_rec; ++i) {
            const int64_t aoff = (int64_t)((uint64_t)rec[0] | ((uint64_t)rec[1] << 32));
            const int x = (int)rec[2];
            const uint32_t n_out = rec[3];
            const size_t step_idx = am.size() - 1 - i;  // (entries: last eliminated first)
            if (x < 0 || x >= n || !in_m[x]) fail(b, "MAX step eliminates variable " + std::to_string(x) + ", which is not in M");
            if (aoff != am[step_idx].first || card[x] != am_cx[step_idx]) fail(b, "traceback entry " + std::to_string(i) + " does not match its MAX step");
            if (known[x]) fail(b, "variable " + std::to_string(x) + " is decoded twice");
            int64_t idx = 0;
            for (uint32_t a = 0; a < n_out; ++a) {
                const uint32_t v = rec[4 + 2 * a];
                if (v >= (uint32_t)n || !in_m[v]) fail(b, "traceback axis " + std::to_string(v) + " is not a MAP variable");
                if (!known[v]) fail(b, "traceback reads variable " + std::to_string(v) + " before it is decoded");
                idx += (int64_t)code[v] * (int64_t)rec[5 + 2 * a];
            }
            if (m > 0) {
                uint16_t v;
                arena_at(aoff + idx / 4);
                std::memcpy(&v, reinterpret_cast<const char *>(arena.data() + aoff) + 2 * idx, 2);
                code[x] = v;
            }
            known[x] = 1;
            rec += 4 + 2 * n_out;
        }
        // gather list
        if ((int)rec[0] != nm) fail(b, "gather list has " + std::to_string(rec[0]) + " entries for " + std::to_string(nm) + " MAP variables");
        for (int k = 0; k < nm; ++k) {
            if ((int32_t)rec[1 + k] != mv[k]) fail(b, "gather list entry " + std::to_string(k) + " is not the caller's");
            if (!known[mv[k]]) fail(b, "MAP variable " + std::to_string(mv[k]) + " is never decoded");
        }
        if (!(m > 0)) { print_zero(); continue; }
        std::printf("%a", std::log(m));
        for (int k = 0; k < nm; ++k) std::printf(" %d", code[rec[1 + k]]);
        std::printf("\n");
    }
    return 0;
}
