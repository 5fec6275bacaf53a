// Host interpreter of MIBN_Q_UNNORMALISED programs (planner.h, "UNNORMALISED requests"): pins the emission of P(q, e) / P(e)
// requests independently of the kernels (tests/test_evidence_host.py builds and runs it).
//
//   g++ -O2 -mpopcnt -std=c++17 tools/ev_sim.cpp sorobn_amd/csrc/planner.cpp -lpthread -o ev_sim && ./ev_sim run net.txt
//
// Input (whitespace-separated): n_vars, card[n], scope_off[n + 1], scope_vars[], value_off[n + 1], values[] (any strtod
// format), B, then per request: no_prune (0 / 1), nq, qvars[nq], ne, evars[ne], ecodes[ne].
//
//   run      plans every request with ProgramKind::Raw and runs its program (GENERIC steps only: the small networks' programs).
//            Output: one line per request, its nq-variable table P(q, e) in C-order (%a each; one cell, P(e), for nq = 0).
//            Checks, and exits 1 with a message when one fails: every step is GENERIC, the FINAL step is the last one and
//            carries the RAW flag (and no other step does), every arena access lies inside the request's arena_cells.  A
//            request with an evidence code outside its domain is not planned (the engine skips it): its table is all zero.
//   compare  plans every request (nq >= 1) as ProgramKind::Raw and as Sum: the two programs must be equal word for word but for
//            the RAW bit of the FINAL step.  Output: one line per request, "<words> <steps>".
//   reject   validates every request as ProgramKind::Sum and prints validate_request's message (or "ok"), one line each.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "sim_common.h"

using namespace mibn;

int main(int argc, char **argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: ev_sim run|compare|reject net.txt\n"); return 2; }
    const std::string mode = argv[1];
    if (mode != "run" && mode != "compare" && mode != "reject") { std::fprintf(stderr, "unknown mode %s\n", argv[1]); return 2; }
    slurp(argv[2]);
    Network net;
    read_network(net);
    const std::vector<int32_t> &card = net.card;
    const int64_t B = geti();
    for (int64_t b = 0; b < B; ++b) {
        const bool no_prune = geti() != 0;
        const int nq = (int)geti();
        std::vector<int32_t> qv(nq);
        for (auto &v : qv) v = (int32_t)geti();
        const int ne = (int)geti();
        std::vector<int32_t> ev(ne), ec(ne);
        for (auto &v : ev) v = (int32_t)geti();
        for (auto &c : ec) c = (int32_t)geti();
        Request rq;
        rq.nq = nq;
        rq.qvars = qv.data();
        rq.ne = ne;
        rq.evars = ev.data();
        rq.ecodes = ec.data();
        rq.no_prune = no_prune;
        if (mode == "reject") {
            const std::string ve = validate_request(net, rq);
            std::printf("%s\n", ve.empty() ? "ok" : ve.c_str());
            continue;
        }
        rq.kind = ProgramKind::Raw;
        const std::string ve = validate_request(net, rq);
        if (!ve.empty()) fail(b, ve);
        int64_t qcells = 1;
        for (int i = 0; i < nq; ++i) qcells *= card[qv[i]];
        bool out_of_domain = false;
        for (int i = 0; i < ne; ++i) out_of_domain = out_of_domain || ec[i] < 0 || ec[i] >= card[ev[i]];
        if (mode == "compare") {
            std::vector<uint32_t> p_raw, p_norm;
            PlanStats s1, s2;
            std::string pe = plan_request(net, rq, p_raw, s1);
            if (!pe.empty()) fail(b, pe);
            rq.kind = ProgramKind::Sum;
            pe = plan_request(net, rq, p_norm, s2);
            if (!pe.empty()) fail(b, pe);
            if (p_raw.size() != p_norm.size()) fail(b, "programs of different length");
            size_t off = 1, last = 0;
            for (uint32_t s = 0; s < p_norm[0]; ++s) { last = off; off += p_norm[off + 6]; }
            for (size_t i = 0; i < p_raw.size(); ++i) {
                const uint32_t want = i == last + 1 ? (p_norm[i] | (kFlagRaw << 16)) : p_norm[i];
                if (p_raw[i] != want) fail(b, "word " + std::to_string(i) + " differs");
            }
            if (!((p_norm[last + 1] >> 16) & kFlagFinal) || ((p_norm[last + 1] >> 16) & kFlagRaw)) fail(b, "the last step is not a plain FINAL step");
            if (s1.alg_bytes != s2.alg_bytes || s1.arena_cells != s2.arena_cells) fail(b, "statistics differ");
            std::printf("%zu %u\n", p_raw.size(), p_norm[0]);
            continue;
        }
        std::vector<double> result((size_t)qcells, 0.0);
        if (!out_of_domain) {
            std::vector<uint32_t> prog;
            PlanStats st;
            const std::string pe = plan_request(net, rq, prog, st);
            if (!pe.empty()) fail(b, pe);
            std::vector<double> arena((size_t)std::max<int64_t>(16, st.arena_cells), std::nan(""));
            auto arena_at = [&](int64_t i) -> double & {
                if (i < 0 || i >= (int64_t)arena.size()) fail(b, "arena access " + std::to_string(i) + " outside " + std::to_string(arena.size()) + " cells");
                return arena[(size_t)i];
            };
            const uint32_t n_steps = prog[0];
            if (!n_steps) fail(b, "empty program");
            size_t off = 1;
            for (uint32_t s = 0; s < n_steps; ++s) {
                const GenericStep g(b, s, prog.data() + off);
                const uint32_t flags = g.flags;
                const bool fin = flags & kFlagFinal, raw = flags & kFlagRaw;
                if (fin != (s + 1 == n_steps)) fail(b, "FINAL flag on step " + std::to_string(s) + " of " + std::to_string(n_steps));
                if (raw != fin) fail(b, "RAW flag on step " + std::to_string(s) + " does not match its FINAL flag");
                if (flags & kFlagMax) fail(b, "MAX flag in a sum program");
                const int64_t cells = g.cells, out_off = g.out_off;
                if (fin && (cells != qcells || out_off != 0)) fail(b, "FINAL step of " + std::to_string(cells) + " cells at " + std::to_string(out_off));
                std::vector<double> outv((size_t)cells, 0.0);
                g.visit(net, arena_at, [&](int64_t o, int, double prod) { outv[(size_t)o] += prod; });  // sum over x
                for (int64_t o = 0; o < cells; ++o) {
                    if (fin) result[(size_t)o] = outv[(size_t)o];
                    else arena_at(out_off + o) = outv[(size_t)o];
                }
                off += g.words;
            }
        }
        for (int64_t c = 0; c < qcells; ++c) std::printf(c ? " %a" : "%a", result[(size_t)c]);
        std::printf("\n");
    }
    return 0;
}
