// Host interpreter of max programs (planner.h, "MAX programs") and of their traceback records: pins the emission of
// mibn_mpe_batch independently of the kernels (tests/test_mpe_host.py builds and runs it).
//
//   g++ -O2 -mpopcnt -std=c++17 tools/max_sim.cpp sorobn_amd/csrc/planner.cpp -lpthread -o max_sim && ./max_sim net.txt
//
// Input (whitespace-separated): n_vars, card[n], scope_off[n + 1], scope_vars[], value_off[n + 1], values[] (any strtod
// format), B, then per request: ne, evars[ne], ecodes[ne].  Output: one line per request, "log_p code_0 .. code_{n-1}"
// (log_p as %a, or -inf).  Besides running the programs it checks, and exits 1 with a message when one fails:
//   * every step is GENERIC;
//   * a step that eliminates a variable (cx > 1) carries the MAX flag, and the record has one entry per such step;
//   * the argmax tables of a request do not overlap each other nor an intermediate while it is live;
//   * every arena access lies inside the request's arena_cells.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "sim_common.h"

using namespace mibn;

int main(int argc, char **argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: max_sim net.txt\n"); return 2; }
    slurp(argv[1]);
    Network net;
    read_network(net);
    const int n = net.n_vars;
    const std::vector<int32_t> &card = net.card;
    const int64_t B = geti();
    for (int64_t b = 0; b < B; ++b) {
        const int ne = (int)geti();
        std::vector<int32_t> ev(ne), ec(ne);
        for (auto &v : ev) v = (int32_t)geti();
        for (auto &c : ec) c = (int32_t)geti();
        std::vector<int32_t> code(n, 0);
        bool out_of_domain = false;
        for (int i = 0; i < ne; ++i) out_of_domain = out_of_domain || ec[i] < 0 || ec[i] >= card[ev[i]];
        if (out_of_domain) {  // (the engine skips such a request: zero probability)
            for (int v = 0; v < n; ++v) code[v] = -1;
            for (int i = 0; i < ne; ++i) code[ev[i]] = ec[i];
            std::printf("-inf");
            for (int v = 0; v < n; ++v) std::printf(" %d", code[v]);
            std::printf("\n");
            continue;
        }
        Request rq;
        rq.ne = ne;
        rq.evars = ev.data();
        rq.ecodes = ec.data();
        rq.kind = ProgramKind::Max;
        const std::string ve = validate_mpe_request(net, rq);
        if (!ve.empty()) fail(b, ve);
        std::vector<uint32_t> prog;
        PlanStats st;
        const std::string pe = plan_request(net, rq, prog, st);
        if (!pe.empty()) fail(b, pe);
        std::vector<double> arena((size_t)std::max<int64_t>(16, st.arena_cells), std::nan(""));
        double m = 0;
        struct Table { int64_t off, cells; int written, last_read; };
        std::vector<Table> tabs;                    // intermediates
        std::vector<std::pair<int64_t, int64_t>> am;  // argmax regions (doubles)
        auto arena_at = [&](int64_t i) -> double & {
            if (i < 0 || i >= (int64_t)arena.size()) fail(b, "arena access " + std::to_string(i) + " outside " + std::to_string(arena.size()) + " cells");
            return arena[(size_t)i];
        };
        const uint32_t n_steps = prog[0];
        size_t off = 1;
        int n_flagged = 0;
        for (uint32_t s = 0; s < n_steps; ++s) {
            const GenericStep g(b, s, prog.data() + off);
            const int n_in = g.n_in, cx = g.cx;
            const bool fin = g.flags & kFlagFinal, mx = g.flags & kFlagMax;
            if (cx > 1 && !mx) fail(b, "elimination step " + std::to_string(s) + " without the MAX flag");
            if (cx <= 1 && mx) fail(b, "product step " + std::to_string(s) + " with the MAX flag");
            const int64_t cells = g.cells, out_off = g.out_off;
            const std::vector<uint64_t> &in_off = g.in_off;
            // reads of intermediates
            for (int j = 0; j < n_in; ++j)
                if (!(in_off[j] & kConstFlag))
                    for (size_t t = tabs.size(); t-- > 0;)
                        if (tabs[t].off == (int64_t)in_off[j]) { tabs[t].last_read = (int)s; break; }
            const int64_t am_off = g.am_off;
            if (mx) {
                ++n_flagged;
                const int64_t am_cells = (cells * 2 + 7) / 8;
                for (auto &r : am)
                    if (am_off < r.first + r.second && r.first < am_off + am_cells) fail(b, "argmax tables overlap");
                am.push_back({am_off, am_cells});
                arena_at(am_off + am_cells - 1);
            }
            if (!fin) tabs.push_back({out_off, cells, (int)s, (int)s});
            std::vector<double> outv((size_t)cells);
            std::vector<uint16_t> arg((size_t)cells);
            g.visit(net, arena_at, [&](int64_t o, int x, double prod) {  // max over x, the lowest x that attains it
                if (x == 0 || prod > outv[(size_t)o]) { outv[(size_t)o] = prod; arg[(size_t)o] = (uint16_t)x; }
            });
            for (int64_t o = 0; o < cells; ++o) {
                if (fin) { if (cells != 1 || out_off != 0) fail(b, "FINAL step of more than one cell"); m = outv[0]; }
                else arena_at(out_off + o) = outv[(size_t)o];
            }
            if (mx) std::memcpy(reinterpret_cast<char *>(arena.data() + am_off), arg.data(), (size_t)cells * 2);
            off += g.words;
        }
        // live intermediates against argmax tables: a table written at step s and last read at step t is live over [s, t]; the argmax
        // table of step k must not overlap it when s <= k <= t (nor may a later intermediate overwrite an argmax table)
        {
            size_t o2 = 1;
            std::vector<int> am_step;
            for (uint32_t s = 0; s < n_steps; ++s) {
                const uint32_t *w = prog.data() + o2;
                if ((w[1] >> 16) & kFlagMax) am_step.push_back((int)s);
                o2 += w[6];
            }
            for (size_t a = 0; a < am.size(); ++a)
                for (const Table &t : tabs) {
                    const bool overlap = am[a].first < t.off + t.cells && t.off < am[a].first + am[a].second;
                    if (overlap && (t.written >= am_step[a] || t.last_read >= am_step[a]))
                        fail(b, "argmax table of step " + std::to_string(am_step[a]) + " overlaps a live intermediate");
                }
        }
        // traceback
        const uint32_t *rec = prog.data() + off;
        const uint32_t n_rec = rec[0], n_ev = rec[1];
        if ((int)n_rec != n_flagged) fail(b, "traceback record has " + std::to_string(n_rec) + " entries for " + std::to_string(n_flagged) + " elimination steps");
        rec += 2;
        for (uint32_t i = 0; i < n_ev; ++i) code[rec[2 * i]] = (int32_t)rec[2 * i + 1];
        rec += 2 * n_ev;
        std::vector<char> known(n, 1);
        {
            const uint32_t *r2 = rec;
            for (uint32_t i = 0; i < n_rec; ++i) { known[r2[2]] = 0; r2 += 4 + 2 * r2[3]; }
        }
        if (m > 0) {
            for (uint32_t i = 0; i < n_rec; ++i) {
                const int64_t aoff = (int64_t)((uint64_t)rec[0] | ((uint64_t)rec[1] << 32));
                const int x = (int)rec[2];
                const uint32_t n_out = rec[3];
                int64_t idx = 0;
                for (uint32_t a = 0; a < n_out; ++a) {
                    if (!known[rec[4 + 2 * a]]) fail(b, "traceback reads variable " + std::to_string(rec[4 + 2 * a]) + " before it is decoded");
                    idx += (int64_t)code[rec[4 + 2 * a]] * (int64_t)rec[5 + 2 * a];
                }
                uint16_t v;
                arena_at(aoff + idx / 4);
                std::memcpy(&v, reinterpret_cast<const char *>(arena.data() + aoff) + 2 * idx, 2);
                code[x] = v;
                known[x] = 1;
                rec += 4 + 2 * n_out;
            }
            std::printf("%a", std::log(m));
        } else {
            for (int v = 0; v < n; ++v) code[v] = -1;
            for (int i = 0; i < ne; ++i) code[ev[i]] = ec[i];
            std::printf("-inf");
        }
        for (int v = 0; v < n; ++v) std::printf(" %d", code[v]);
        std::printf("\n");
    }
    return 0;
}
