// What the host twins of the three program flavours share (max_sim.cpp, ev_sim.cpp, draw_sim.cpp): the token reader over their
// input file, the network prefix of the three input formats, and the one decoder / evaluator of a GENERIC step (planner.h, "Step
// encoding").  Everything specific to a flavour - its flag checks, its reduction over the eliminated variable, its record - stays
// in its own file.
#pragma once

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../sorobn_amd/csrc/planner.h"

static std::vector<char> g_in;
static size_t g_pos = 0;

// the whole input file, tokenised in place by next_tok
static void slurp(const char *path) {
    FILE *f = std::fopen(path, "rb");
    if (!f) { std::perror(path); std::exit(2); }
    char buf[1 << 16];
    size_t k;
    while ((k = std::fread(buf, 1, sizeof buf, f)) > 0) g_in.insert(g_in.end(), buf, buf + k);
    std::fclose(f);
    g_in.push_back(0);
}
static const char *next_tok() {
    while (g_pos < g_in.size() && (g_in[g_pos] == ' ' || g_in[g_pos] == '\n' || g_in[g_pos] == '\t' || g_in[g_pos] == '\r')) ++g_pos;
    if (g_pos >= g_in.size()) { std::fprintf(stderr, "input ends early\n"); std::exit(2); }
    const char *t = g_in.data() + g_pos;
    while (g_pos < g_in.size() && !(g_in[g_pos] == ' ' || g_in[g_pos] == '\n' || g_in[g_pos] == '\t' || g_in[g_pos] == '\r')) ++g_pos;
    if (g_pos < g_in.size()) g_in[g_pos++] = 0;
    return t;
}
static int64_t geti() { return std::strtoll(next_tok(), nullptr, 10); }
[[maybe_unused]] static uint64_t getu() { return std::strtoull(next_tok(), nullptr, 10); }
static double getd() { return std::strtod(next_tok(), nullptr); }

[[noreturn]] static void fail(int64_t b, const std::string &m) {
    std::fprintf(stderr, "request %lld: %s\n", (long long)b, m.c_str());
    std::exit(1);
}

// The prefix common to the three input formats: n_vars, card[n], scope_off[n + 1], scope_vars[], value_off[n + 1], values[].
static void read_network(mibn::Network &net) {
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
    const std::string e = net.set(n, card.data(), scope_off.data(), scope_vars.data(), value_off.data(), values.data());
    if (!e.empty()) { std::fprintf(stderr, "set: %s\n", e.c_str()); std::exit(2); }
}

// A GENERIC step as its words say (emit_core.h, emit_generic): psi[o] = reduce_x prod_j phi_j[o0_j(o) + x * xs_j].
struct GenericStep {
    int n_in, na, cx;
    uint32_t flags;
    int64_t cells, out_off;
    int64_t am_off = -1;  // the argmax table (kFlagMax only)
    uint32_t words;       // length of the step: the next one starts `words` further
    std::vector<uint64_t> in_off;  // arena offset, or pool offset | kConstFlag
    std::vector<int64_t> xs;
    const uint32_t *cd;    // [na] extents of the output axes, fastest first
    const int32_t *strd;   // [n_in][na] stride of input j along output axis a

    // step s of request b, at w: any other kind of step fails the request
    GenericStep(int64_t b, uint32_t s, const uint32_t *w) {
        if ((w[0] & 0xff) != mibn::kKindGeneric) fail(b, "step " + std::to_string(s) + " is not GENERIC");
        n_in = (w[0] >> 8) & 0xff;
        na = (w[0] >> 16) & 0xff;
        cx = (int)(w[1] & 0xffff);
        flags = w[1] >> 16;
        cells = (int64_t)w[2] * (int64_t)w[3];
        out_off = (int64_t)((uint64_t)w[4] | ((uint64_t)w[5] << 32));
        words = w[6];
        if (flags & mibn::kFlagMax) am_off = (int64_t)((uint64_t)w[7] | ((uint64_t)w[8] << 32));
        const uint32_t *p = w + mibn::kHdrWords;
        in_off.resize((size_t)n_in);
        xs.resize((size_t)n_in);
        for (int j = 0; j < n_in; ++j) { in_off[j] = (uint64_t)p[3 * j] | ((uint64_t)p[3 * j + 1] << 32); xs[j] = (int32_t)p[3 * j + 2]; }
        cd = p + 3 * n_in;
        strd = (const int32_t *)(cd + na);
    }

    // term(o, x, prod) for every output cell o in ascending order and, within a cell, x = 0 .. max(1, cx) - 1: prod is the product
    // over the inputs in ascending j, starting from 1 (no input: the empty product).  Constants come from net.pool, intermediates
    // through arena_at (the caller's bounds-checked arena).  The caller reduces over x; the order of the multiplications and of the
    // x loop is fixed - draw_sim is compared with the device at the level of which state a uniform selects.
    template <class ArenaAt, class Term>
    void visit(const mibn::Network &net, ArenaAt &&arena_at, Term &&term) const {
        std::vector<int64_t> o0((size_t)n_in);
        for (int64_t o = 0; o < cells; ++o) {
            int64_t r = o;
            for (int j = 0; j < n_in; ++j) o0[j] = 0;
            for (int a = 0; a < na; ++a) {
                const int64_t d = r % cd[a];
                r /= cd[a];
                for (int j = 0; j < n_in; ++j) o0[j] += d * strd[j * na + a];
            }
            for (int x = 0; x < std::max(1, cx); ++x) {
                double prod = 1;
                for (int j = 0; j < n_in; ++j) {
                    const int64_t i = o0[j] + x * xs[j];
                    prod *= (in_off[j] & mibn::kConstFlag) ? net.pool[(size_t)((in_off[j] & ~mibn::kConstFlag) + i)] : arena_at((int64_t)in_off[j] + i);
                }
                term(o, x, prod);
            }
        }
    }
};
