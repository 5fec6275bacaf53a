// Host interpreter of MIBN_Q_UNNORMALISED programs (planner.h, "UNNORMALISED requests"): pins the emission of P(q, e) / P(e)
// requests independently of the kernels (tests/test_evidence_host.py builds and runs it).
//
//   g++ -O2 -mpopcnt -std=c++17 tools/ev_sim.cpp sorobn_amd/csrc/planner.cpp -lpthread -o ev_sim && ./ev_sim run net.txt
//
// Input (whitespace-separated): n_vars, card[n], scope_off[n + 1], scope_vars[], value_off[n + 1], values[] (any strtod
// format), B, then per request: no_prune (0 / 1), nq, qvars[nq], ne, evars[ne], ecodes[ne].
//
//   run      plans every request with Request::raw and runs its program (GENERIC steps only: the small networks' programs).
//            Output: one line per request, its nq-variable table P(q, e) in C-order (%a each; one cell, P(e), for nq = 0).
//            Checks, and exits 1 with a message when one fails: every step is GENERIC, the FINAL step is the last one and
//            carries the RAW flag (and no other step does), every arena access lies inside the request's arena_cells.  A
//            request with an evidence code outside its domain is not planned (the engine skips it): its table is all zero.
//   compare  plans every request (nq >= 1) with and without Request::raw: the two programs must be equal word for word but for
//            the RAW bit of the FINAL step.  Output: one line per request, "<words> <steps>".
//   reject   validates every request without Request::raw and prints validate_request's message (or "ok"), one line each.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../sorobn_amd/csrc/planner.h"

using namespace mibn;

static std::vector<char> g_in;
static size_t g_pos = 0;
static const char *next_tok() {
    while (g_pos < g_in.size() && (g_in[g_pos] == ' ' || g_in[g_pos] == '\n' || g_in[g_pos] == '\t' || g_in[g_pos] == '\r')) ++g_pos;
    if (g_pos >= g_in.size()) { std::fprintf(stderr, "input ends early\n"); std::exit(2); }
    const char *t = g_in.data() + g_pos;
    while (g_pos < g_in.size() && !(g_in[g_pos] == ' ' || g_in[g_pos] == '\n' || g_in[g_pos] == '\t' || g_in[g_pos] == '\r')) ++g_pos;
    if (g_pos < g_in.size()) g_in[g_pos++] = 0;
    return t;
}
static int64_t geti() { return std::strtoll(next_tok(), nullptr, 10); }
static double getd() { return std::strtod(next_tok(), nullptr); }

[[noreturn]] static void fail(int64_t b, const std::string &m) {
    std::fprintf(stderr, "request %lld: %s\n", (long long)b, m.c_str());
    std::exit(1);
}

int main(int argc, char **argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: ev_sim run|compare|reject net.txt\n"); return 2; }
    const std::string mode = argv[1];
    if (mode != "run" && mode != "compare" && mode != "reject") { std::fprintf(stderr, "unknown mode %s\n", argv[1]); return 2; }
    FILE *f = std::fopen(argv[2], "rb");
    if (!f) { std::perror(argv[2]); return 2; }
    char buf[1 << 16];
    size_t k;
    while ((k = std::fread(buf, 1, sizeof buf, f)) > 0) g_in.insert(g_in.end(), buf, buf + k);
    std::fclose(f);
    g_in.push_back(0);
    const int n = (int)geti();
    std::vector<int32_t> card(n), scope_vars;
    std::vector<int64_t> scope_off(n + 1), value_off(n + 1);
    for (auto &c : card) c = (int32_t)geti();
    for (auto &o : scope_off) o = geti();
    scope_vars.resize((size_t)scope_off[n]);
    for (auto &v : scope_vars) v = (int32_t)geti();
    for (auto &o : value_off) o = geti();
    std::vector<double> values((size_t)value_off[n]);
    for (auto &v : values) v = getd();
    Network net;
    const std::string e = net.set(n, card.data(), scope_off.data(), scope_vars.data(), value_off.data(), values.data());
    if (!e.empty()) { std::fprintf(stderr, "set: %s\n", e.c_str()); return 2; }
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
        rq.raw = true;
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
            rq.raw = false;
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
                const uint32_t *w = prog.data() + off;
                if ((w[0] & 0xff) != kKindGeneric) fail(b, "step " + std::to_string(s) + " is not GENERIC");
                const int n_in = (w[0] >> 8) & 0xff, na = (w[0] >> 16) & 0xff;
                const int cx = (int)(w[1] & 0xffff);
                const uint32_t flags = w[1] >> 16;
                const bool fin = flags & kFlagFinal, raw = flags & kFlagRaw;
                if (fin != (s + 1 == n_steps)) fail(b, "FINAL flag on step " + std::to_string(s) + " of " + std::to_string(n_steps));
                if (raw != fin) fail(b, "RAW flag on step " + std::to_string(s) + " does not match its FINAL flag");
                if (flags & kFlagMax) fail(b, "MAX flag in a sum program");
                const int64_t cells = (int64_t)w[2] * (int64_t)w[3];
                const int64_t out_off = (int64_t)((uint64_t)w[4] | ((uint64_t)w[5] << 32));
                if (fin && (cells != qcells || out_off != 0)) fail(b, "FINAL step of " + std::to_string(cells) + " cells at " + std::to_string(out_off));
                const uint32_t *p = w + kHdrWords;
                std::vector<uint64_t> in_off(n_in);
                std::vector<int64_t> xs(n_in);
                for (int j = 0; j < n_in; ++j) { in_off[j] = (uint64_t)p[3 * j] | ((uint64_t)p[3 * j + 1] << 32); xs[j] = (int32_t)p[3 * j + 2]; }
                const uint32_t *cd = p + 3 * n_in;
                const int32_t *strd = (const int32_t *)(cd + na);
                std::vector<double> outv((size_t)cells);
                std::vector<int64_t> o0(n_in);
                for (int64_t o = 0; o < cells; ++o) {
                    int64_t r = o;
                    for (int j = 0; j < n_in; ++j) o0[j] = 0;
                    for (int a = 0; a < na; ++a) {
                        const int64_t d = r % cd[a];
                        r /= cd[a];
                        for (int j = 0; j < n_in; ++j) o0[j] += d * strd[j * na + a];
                    }
                    double acc = 0;
                    for (int x = 0; x < std::max(1, cx); ++x) {
                        double prod = 1;  // (no input: the empty product)
                        for (int j = 0; j < n_in; ++j) {
                            const int64_t i = o0[j] + x * xs[j];
                            prod *= (in_off[j] & kConstFlag) ? net.pool[(size_t)((in_off[j] & ~kConstFlag) + i)] : arena_at((int64_t)in_off[j] + i);
                        }
                        acc += prod;
                    }
                    outv[(size_t)o] = acc;
                }
                for (int64_t o = 0; o < cells; ++o) {
                    if (fin) result[(size_t)o] = outv[(size_t)o];
                    else arena_at(out_off + o) = outv[(size_t)o];
                }
                off += w[6];
            }
        }
        for (int64_t c = 0; c < qcells; ++c) std::printf(c ? " %a" : "%a", result[(size_t)c]);
        std::printf("\n");
    }
    return 0;
}
