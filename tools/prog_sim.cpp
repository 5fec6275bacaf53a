// Host interpreter of the step-wise program kinds (planner.h: MAX, MAP, DRAW programs and UNNORMALISED requests), of their
// traceback records, gather lists and draw records: pins the emission of mibn_mpe_batch, mibn_map_batch,
// mibn_posterior_sample_batch and MIBN_Q_UNNORMALISED independently of the kernels.  One binary, one sub-command per kind
// (tests/sim_tools.py builds it once per test session; tests/test_{mpe,map,posterior_sampling,evidence}_host.py run it, and
// tests/test_posterior_sampling.py compares the device with `draw` row for row).
//
//   g++ -O2 -mpopcnt -std=c++17 -ffp-contract=off tools/prog_sim.cpp sorobn_amd/csrc/planner.cpp -lpthread -o prog_sim
//   ./prog_sim max net.txt | map net.txt | draw net.txt codes.bin [margins.bin] | ev run|compare|reject net.txt
//   options, anywhere on the command line (none: a bare Network, as before): --small_cells N --big_iters N --tile_h N
//   --order_effort N --second_above X --minfill_above X --hints FILE (n_hints, then n_hints x n_vars priorities) - the planner
//   options of an engine, so that the program run here is the engine's word for word (the order search reads them, and the order
//   decides which of two equal maxima a traceback meets first); --ties (max, map): one line per planned request on standard
//   error, "ties <request> <cells> <on_path>" - the output cells of MAX steps whose maximum two or more x attain with bitwise equal
//   positive products, and how many of them the traceback reads.
//   --lh FILE (max, map, ev run): likelihood findings (planner.h), whitespace-separated - per request of the
//   input, in order: its number of findings, then for each the variable id and one weight per state of it (any strtod format).  The
//   request formats on standard input do not change.  The interpreter writes the seeds into its NaN-filled arena before the first
//   step, where emit_begin put them - a seed read at a wrong offset is a NaN in the result - and fails a request whose step writes
//   its output or its argmax table over a seed; the seeds are intermediates written "before step 0" in the liveness checks.
//   --dump: one line per planned request on standard error, "prog <request> <arena_cells> <seed_cells> <word> ..": the program.
//
// (-ffp-contract=off: `draw` is the CPU twin of the draw kernel - same programs, same Philox4x32-10 stream, same arithmetic.)
// tools/max_sim.cpp, map_sim.cpp, draw_sim.cpp and ev_sim.cpp are three lines each: this file with the kind fixed (PROG_SIM_KIND),
// so that the build lines and command lines of the former stand-alone twins (`max_sim net.txt`, `ev_sim run net.txt`, ..) still work.
//
// Input (whitespace-separated): n_vars, card[n], scope_off[n + 1], scope_vars[], value_off[n + 1], values[] (any strtod format),
// then what the kind reads.  What every kind shares appears once below: the request reader, the out-of-domain short cut (the
// engine skips such a request: zero probability), planning, the NaN-filled bounds-checked arena, ONE step loop - it runs the
// program as written: a step flagged MAX maximises (the lowest x that attains the maximum goes to its argmax table), any other
// step sums -, one check of the argmax tables and one traceback decode.  Every failed check exits 1 with a message.  Checked for
// every kind: every step is GENERIC; every arena access lies inside the request's arena_cells.  Each kind keeps its own rules:
//
//   max    B, then per request: ne, evars[ne], ecodes[ne].  Output: one line per request, "log_p code_0 .. code_{n-1}" (log_p as
//          %a, or -inf).  Checks:
//            * a step that eliminates a variable (cx > 1) carries the MAX flag, and the record has one entry per such step;
//            * the argmax tables of a request do not overlap each other nor an intermediate while it is live.
//   map    B, then per request: no_prune (0 / 1), nm, mvars[nm], ne, evars[ne], ecodes[ne].  Output: one line per request,
//          "log_p code_0 .. code_{nm-1}" (log_p as %a, or -inf; the codes of mvars in the order given).  Checks:
//            * no unflagged step eliminates a variable (cx > 1) after the first MAX step; no product-only step carries the flag;
//            * the record has one entry per MAX step, and every MAX step eliminates a variable of M (the entry's variable, of the
//              step's cx);
//            * the argmax tables of a request overlap neither each other nor an intermediate while it is live;
//            * every axis of a traceback entry is a MAP variable decoded before it is used;
//            * the gather list is M in the caller's order.
//   draw   seed, prune (0 / 1), B, then per request: ne, evars[ne], ecodes[ne], n_samples, g_first (the global row index of its
//          first sample: the Philox counter).  codes.bin receives the rows of all requests, int32[n_vars] each, in request order;
//          margins.bin (optional) one double per row: the smallest margin of its draws, min_x |u * total - acc_x| / total - how
//          far the nearest boundary of the running sum was from the uniform.  Standard output, one line per request:
//            p_e (%a)  n_steps  n_back  n_fwd  kept_cells  smallest margin (%a)  k  g_1 .. g_k   (the k rows of margin <= 1e-12)
//          Checks:
//            * no step carries the MAX flag, the FINAL step is one cell and carries the RAW flag;
//            * no table of a request overlaps another one (nothing is released: every intermediate lives until the draw), and
//              PlanStats::kept_cells accounts for all of them;
//            * the record has one backward entry per elimination step, and every variable a draw reads is evidence or drawn before;
//            * a draw never meets a zero total when the mass is positive.
//   ev     B, then per request: no_prune (0 / 1), nq, qvars[nq], ne, evars[ne], ecodes[ne].
//          run      plans every request with ProgramKind::Raw and runs its program (GENERIC steps only: the small networks'
//                   programs).  Output: one line per request, its nq-variable table P(q, e) in C-order (%a each; one cell, P(e),
//                   for nq = 0).  Checks: the FINAL step is the last one and carries the RAW flag (and no other step does), no
//                   step carries the MAX flag.  A request with an evidence code outside its domain is not planned: all zero.
//          compare  plans every request (nq >= 1) as ProgramKind::Raw and as Sum: the two programs must be equal word for word
//                   but for the RAW bit of the FINAL step.  Output: one line per request, "<words> <steps>".
//          reject   validates every request as ProgramKind::Sum and prints validate_request's message (or "ok"), one line each.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../sorobn_amd/csrc/planner.h"

using namespace mibn;

// ------------------------------------------------------------------------------------------------------------------ the reader
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
static uint64_t getu() { return std::strtoull(next_tok(), nullptr, 10); }
static double getd() { return std::strtod(next_tok(), nullptr); }

[[noreturn]] static void fail(int64_t b, const std::string &m) {
    std::fprintf(stderr, "request %lld: %s\n", (long long)b, m.c_str());
    std::exit(1);
}

// The prefix common to every input format: n_vars, card[n], scope_off[n + 1], scope_vars[], value_off[n + 1], values[].
static void read_network(Network &net) {
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

enum class Kind { Max, Map, Draw, Ev };

// One request as its kind's input format gives it: [no_prune, nq, qvars] (map, ev), ne, evars, ecodes, [n_samples, g_first] (draw).
struct Query {
    bool no_prune = false;
    std::vector<int32_t> qv, ev, ec;
    std::vector<int32_t> lv;              // --lh: the finding variables of the request
    std::vector<std::vector<double>> lw;  // ... and their weights
    int64_t n_samples = 0;
    uint64_t g_first = 0;

    Query(Kind kind, bool no_prune_) : no_prune(no_prune_) {
        if (kind == Kind::Map || kind == Kind::Ev) {
            no_prune = geti() != 0;
            qv.resize((size_t)geti());
            for (auto &v : qv) v = (int32_t)geti();
        }
        ev.resize((size_t)geti());
        ec.resize(ev.size());
        for (auto &v : ev) v = (int32_t)geti();
        for (auto &c : ec) c = (int32_t)geti();
        if (kind == Kind::Draw) { n_samples = geti(); g_first = getu(); }
    }
    Request request(ProgramKind kind) const {
        Request rq;
        rq.nq = (int32_t)qv.size();
        rq.qvars = qv.data();
        rq.ne = (int32_t)ev.size();
        rq.evars = ev.data();
        rq.ecodes = ec.data();
        rq.kind = kind;
        rq.no_prune = no_prune;
        rq.nl = (int32_t)lv.size();
        rq.lvars = lv.data();
        return rq;
    }
    // (the engine skips such a request: zero probability)
    bool out_of_domain(const Network &net) const {
        bool out = false;
        for (size_t i = 0; i < ev.size(); ++i) out = out || ec[i] < 0 || ec[i] >= net.card[ev[i]];
        return out;
    }
};

// ------------------------------------------------------------------------------------------------------------- the interpreter
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
        if ((w[0] & 0xff) != kKindGeneric) fail(b, "step " + std::to_string(s) + " is not GENERIC");
        n_in = (w[0] >> 8) & 0xff;
        na = (w[0] >> 16) & 0xff;
        cx = (int)(w[1] & 0xffff);
        flags = w[1] >> 16;
        cells = (int64_t)w[2] * (int64_t)w[3];
        out_off = (int64_t)((uint64_t)w[4] | ((uint64_t)w[5] << 32));
        words = w[6];
        if (flags & kFlagMax) am_off = (int64_t)((uint64_t)w[7] | ((uint64_t)w[8] << 32));
        const uint32_t *p = w + kHdrWords;
        in_off.resize((size_t)n_in);
        xs.resize((size_t)n_in);
        for (int j = 0; j < n_in; ++j) { in_off[j] = (uint64_t)p[3 * j] | ((uint64_t)p[3 * j + 1] << 32); xs[j] = (int32_t)p[3 * j + 2]; }
        cd = p + 3 * n_in;
        strd = (const int32_t *)(cd + na);
    }

    // term(o, x, prod) for every output cell o in ascending order and, within a cell, x = 0 .. max(1, cx) - 1: prod is the product
    // over the inputs in ascending j, starting from 1 (no input: the empty product).  Constants come from net.pool, intermediates
    // through arena_at (the bounds-checked arena).  The caller reduces over x; the order of the multiplications and of the x loop
    // is fixed - `draw` is compared with the device at the level of which state a uniform selects.
    template <class ArenaAt, class Term>
    void visit(const Network &net, ArenaAt &&arena_at, Term &&term) const {
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
                    prod *= (in_off[j] & kConstFlag) ? net.pool[(size_t)((in_off[j] & ~kConstFlag) + i)] : arena_at((int64_t)in_off[j] + i);
                }
                term(o, x, prod);
            }
        }
    }
};

static bool g_dump = false;

// A planned request and what running it leaves behind.
struct Run {
    int64_t b;
    std::vector<uint32_t> prog;
    PlanStats st;
    std::vector<double> arena;   // arena_cells, NaN until written
    std::vector<double> final_;  // the cells of the FINAL step (empty: no such step ran)
    struct Table { int64_t off, cells; int written, last_read; };
    std::vector<Table> tabs;     // the intermediates
    struct Argmax { int64_t off, cells; int step, cx; std::vector<char> tie; };
    std::vector<Argmax> am;      // the argmax tables (off, cells in doubles) of the MAX steps, in step order; tie[o]: two or more x attain the (positive) maximum of cell o
    int64_t tie_cells = 0, tie_on_path = 0;  // cells with tie set over all MAX steps; those of them a traceback read (--ties)
    int64_t seed_cells = 0;      // the first cells of the arena: the seeds of the request's findings, each padded to 16

    Run(const Network &net, int64_t b_, const Request &rq, const Query &q) : b(b_) {
        const std::string pe = plan_request(net, rq, prog, st);
        if (!pe.empty()) fail(b, pe);
        arena.assign((size_t)std::max<int64_t>(16, st.arena_cells), std::nan(""));
        for (const std::vector<double> &w : q.lw) {  // what likelihood_seed_kernel writes before level 0
            const int64_t cells = (int64_t)w.size();
            if (seed_cells + cells > st.arena_cells) fail(b, "the seeds do not fit arena_cells " + std::to_string(st.arena_cells));
            for (int64_t c = 0; c < cells; ++c) arena[(size_t)(seed_cells + c)] = w[(size_t)c];
            tabs.push_back({seed_cells, cells, -1, -1});
            seed_cells += (cells + 15) & ~int64_t(15);
        }
        if (g_dump) {
            std::fprintf(stderr, "prog %lld %lld %lld", (long long)b, (long long)st.arena_cells, (long long)seed_cells);
            for (uint32_t w : prog) std::fprintf(stderr, " %x", w);
            std::fprintf(stderr, "\n");
        }
    }
    uint32_t n_steps() const { return prog[0]; }
    const uint32_t *record() const { return prog.data() + record_offset(prog.data()); }
    double &at(int64_t i) {
        if (i < 0 || i >= (int64_t)arena.size()) fail(b, "arena access " + std::to_string(i) + " outside " + std::to_string(arena.size()) + " cells");
        return arena[(size_t)i];
    }
    // the FINAL cell of a one-cell program; no step at all: `empty` (the empty product, where the host writes it)
    double mass(double empty) const { return final_.empty() ? (n_steps() ? 0.0 : empty) : final_[0]; }
    uint16_t argmax_at(int64_t aoff, int64_t idx) {
        uint16_t v;
        at(aoff + idx / 4);
        std::memcpy(&v, reinterpret_cast<const char *>(arena.data() + aoff) + 2 * idx, 2);
        return v;
    }

    // The step loop: rules(s, g) is the kind's own check of step s, before it runs.
    template <class Rules>
    void run_steps(const Network &net, Rules &&rules) {
        size_t off = 1;
        for (uint32_t s = 0; s < n_steps(); ++s) {
            const GenericStep g(b, s, prog.data() + off);
            rules(s, g);
            const bool fin = g.flags & kFlagFinal, mx = g.flags & kFlagMax;
            for (int j = 0; j < g.n_in; ++j)  // reads of intermediates
                if (!(g.in_off[j] & kConstFlag))
                    for (size_t t = tabs.size(); t-- > 0;)
                        if (tabs[t].off == (int64_t)g.in_off[j]) { tabs[t].last_read = (int)s; break; }
            if (mx) {
                const int64_t am_cells = (g.cells * 2 + 7) / 8;
                for (const Argmax &r : am)
                    if (g.am_off < r.off + r.cells && r.off < g.am_off + am_cells) fail(b, "argmax tables overlap");
                am.push_back({g.am_off, am_cells, (int)s, g.cx, std::vector<char>((size_t)g.cells, 0)});
                at(g.am_off + am_cells - 1);
                if (g.am_off < seed_cells) fail(b, "the argmax table of step " + std::to_string(s) + " overlaps a seed");
            }
            if (!fin && g.out_off < seed_cells) fail(b, "the output of step " + std::to_string(s) + " overlaps a seed");
            char *tie = mx ? am.back().tie.data() : nullptr;
            if (!fin) tabs.push_back({g.out_off, g.cells, (int)s, (int)s});
            std::vector<double> outv((size_t)g.cells, 0.0);
            std::vector<uint16_t> arg((size_t)g.cells);
            g.visit(net, [&](int64_t i) -> double & { return at(i); }, [&](int64_t o, int x, double prod) {
                if (mx) {  // max over x, the lowest x that attains it
                    if (x == 0 || prod > outv[(size_t)o]) { outv[(size_t)o] = prod; arg[(size_t)o] = (uint16_t)x; tie[o] = 0; }
                    else if (prod == outv[(size_t)o] && prod > 0) tie[o] = 1;
                } else {   // the sum body: 0.0 + the terms in ascending x
                    outv[(size_t)o] += prod;
                }
            });
            if (fin) final_ = outv;
            else for (int64_t o = 0; o < g.cells; ++o) at(g.out_off + o) = outv[(size_t)o];
            if (mx) {
                std::memcpy(reinterpret_cast<char *>(arena.data() + g.am_off), arg.data(), (size_t)g.cells * 2);
                for (int64_t o = 0; o < g.cells; ++o) tie_cells += tie[o];
            }
            off += g.words;
        }
    }

    // A table written at step s and last read at step t is live over [s, t]: the argmax table of step k must not overlap it when
    // s <= k <= t, nor may a later intermediate overwrite an argmax table.
    void check_argmax_liveness() const {
        for (const Argmax &a : am)
            for (const Table &t : tabs) {
                const bool overlap = a.off < t.off + t.cells && t.off < a.off + a.cells;
                if (overlap && (t.written >= a.step || t.last_read >= a.step))
                    fail(b, "argmax table of step " + std::to_string(a.step) + " overlaps a live intermediate");
            }
    }

    // The traceback decode: n_rec entries at rec, last eliminated first - code[x] = argmax[sum_v code[v] * stride_v] where `read`
    // (else the walk only checks).  Every axis must be known by then; entry(i, aoff, x) and axis(v) are the kind's own checks.
    // -> what follows the entries.
    template <class Entry, class Axis>
    const uint32_t *decode(const uint32_t *rec, uint32_t n_rec, bool read, std::vector<int32_t> &code, std::vector<char> &known,
                           Entry &&entry, Axis &&axis) {
        for (uint32_t i = 0; i < n_rec; ++i) {
            const int64_t aoff = (int64_t)((uint64_t)rec[0] | ((uint64_t)rec[1] << 32));
            const int x = (int)rec[2];
            const uint32_t n_out = rec[3];
            entry(i, aoff, x);
            int64_t idx = 0;
            for (uint32_t a = 0; a < n_out; ++a) {
                const uint32_t v = rec[4 + 2 * a];
                axis(v);
                if (!known[v]) fail(b, "traceback reads variable " + std::to_string(v) + " before it is decoded");
                idx += (int64_t)code[v] * (int64_t)rec[5 + 2 * a];
            }
            if (read) {
                code[x] = argmax_at(aoff, idx);
                for (const Argmax &r : am)
                    if (r.off == aoff && idx >= 0 && idx < (int64_t)r.tie.size()) tie_on_path += r.tie[(size_t)idx];
            }
            known[x] = 1;
            rec += 4 + 2 * n_out;
        }
        return rec;
    }
};

static bool g_report_ties = false;
static void report_ties(const Run &R) {
    if (g_report_ties) std::fprintf(stderr, "ties %lld %lld %lld\n", (long long)R.b, (long long)R.tie_cells, (long long)R.tie_on_path);
}

static void one_cell_final(int64_t b, const GenericStep &g) {
    if ((g.flags & kFlagFinal) && (g.cells != 1 || g.out_off != 0)) fail(b, "FINAL step of more than one cell");
}

// ------------------------------------------------------------------------------------------------------------------------- max
static void run_max(const Network &net, int64_t b, const Query &q) {
    const int n = net.n_vars;
    std::vector<int32_t> code(n, 0);
    auto print_codes = [&] {
        for (int v = 0; v < n; ++v) std::printf(" %d", code[v]);
        std::printf("\n");
    };
    auto print_zero = [&] {  // -1 for every non-evidence variable
        for (int v = 0; v < n; ++v) code[v] = -1;
        for (size_t i = 0; i < q.ev.size(); ++i) code[q.ev[i]] = q.ec[i];
        std::printf("-inf");
        print_codes();
    };
    if (q.out_of_domain(net)) { print_zero(); return; }
    const Request rq = q.request(ProgramKind::Max);
    const std::string ve = validate_mpe_request(net, rq);
    if (!ve.empty()) fail(b, ve);
    Run R(net, b, rq, q);
    R.run_steps(net, [&](uint32_t s, const GenericStep &g) {
        const bool mx = g.flags & kFlagMax;
        if (g.cx > 1 && !mx) fail(b, "elimination step " + std::to_string(s) + " without the MAX flag");
        if (g.cx <= 1 && mx) fail(b, "product step " + std::to_string(s) + " with the MAX flag");
        one_cell_final(b, g);
    });
    R.check_argmax_liveness();
    const double m = R.mass(0.0);
    const uint32_t *rec = R.record();
    const uint32_t n_rec = rec[0], n_ev = rec[1];
    if (n_rec != R.am.size()) fail(b, "traceback record has " + std::to_string(n_rec) + " entries for " + std::to_string(R.am.size()) + " elimination steps");
    rec += 2;
    for (uint32_t i = 0; i < n_ev; ++i) code[rec[2 * i]] = (int32_t)rec[2 * i + 1];
    rec += 2 * n_ev;
    if (!(m > 0)) { report_ties(R); print_zero(); return; }
    std::vector<char> known(n, 1);  // (evidence, single-state variables: everything no entry decodes)
    {
        const uint32_t *r2 = rec;
        for (uint32_t i = 0; i < n_rec; ++i) { known[r2[2]] = 0; r2 += 4 + 2 * r2[3]; }
    }
    R.decode(rec, n_rec, true, code, known, [](uint32_t, int64_t, int) {}, [](uint32_t) {});
    report_ties(R);
    std::printf("%a", std::log(m));
    print_codes();
}

// ------------------------------------------------------------------------------------------------------------------------- map
static void run_map(const Network &net, int64_t b, const Query &q) {
    const int n = net.n_vars, nm = (int)q.qv.size();
    const std::vector<int32_t> &card = net.card, &mv = q.qv;
    auto print_zero = [&] {
        std::printf("-inf");
        for (int k = 0; k < nm; ++k) std::printf(" -1");
        std::printf("\n");
    };
    const Request rq = q.request(ProgramKind::Map);
    const std::string ve = validate_request(net, rq);
    if (!ve.empty()) fail(b, ve);
    if (q.out_of_domain(net)) { print_zero(); return; }
    Run R(net, b, rq, q);
    std::vector<char> in_m(n, 0);
    for (int32_t v : mv) in_m[v] = 1;
    bool max_phase = false;
    R.run_steps(net, [&](uint32_t s, const GenericStep &g) {
        const bool fin = g.flags & kFlagFinal, mx = g.flags & kFlagMax;
        if (g.cx <= 1 && mx) fail(b, "product step " + std::to_string(s) + " with the MAX flag");
        if (g.cx > 1 && !mx && max_phase) fail(b, "sum step " + std::to_string(s) + " after the first MAX step");
        if (fin && (s + 1 != R.n_steps() || !(g.flags & kFlagRaw) || g.cx > 1)) fail(b, "FINAL step " + std::to_string(s) + " is not the last, not RAW or eliminates");
        max_phase = max_phase || mx;
        one_cell_final(b, g);
    });
    if (R.n_steps() && R.final_.empty()) fail(b, "no FINAL step");
    R.check_argmax_liveness();
    const double m = R.mass(1.0);
    const uint32_t *rec = R.record();
    const uint32_t n_rec = rec[0], n_ev = rec[1];
    if (n_rec != R.am.size()) fail(b, "traceback record has " + std::to_string(n_rec) + " entries for " + std::to_string(R.am.size()) + " MAX steps");
    if (n_ev != q.ev.size()) fail(b, "traceback record names " + std::to_string(n_ev) + " evidence variables");
    rec += 2 + 2 * n_ev;
    std::vector<int32_t> code(n, 0);
    std::vector<char> known(n, 0);
    for (int v = 0; v < n; ++v) known[v] = in_m[v] && card[v] <= 1;  // (a single-state MAP variable is never eliminated: code 0)
    rec = R.decode(rec, n_rec, m > 0, code, known,
        [&](uint32_t i, int64_t aoff, int x) {
            const Run::Argmax &a = R.am[R.am.size() - 1 - i];  // (entries: last eliminated first)
            if (x < 0 || x >= n || !in_m[x]) fail(b, "MAX step eliminates variable " + std::to_string(x) + ", which is not in M");
            if (aoff != a.off || card[x] != a.cx) fail(b, "traceback entry " + std::to_string(i) + " does not match its MAX step");
            if (known[x]) fail(b, "variable " + std::to_string(x) + " is decoded twice");
        },
        [&](uint32_t v) {
            if (v >= (uint32_t)n || !in_m[v]) fail(b, "traceback axis " + std::to_string(v) + " is not a MAP variable");
        });
    // gather list
    if ((int)rec[0] != nm) fail(b, "gather list has " + std::to_string(rec[0]) + " entries for " + std::to_string(nm) + " MAP variables");
    for (int k = 0; k < nm; ++k) {
        if ((int32_t)rec[1 + k] != mv[k]) fail(b, "gather list entry " + std::to_string(k) + " is not the caller's");
        if (!known[mv[k]]) fail(b, "MAP variable " + std::to_string(mv[k]) + " is never decoded");
    }
    report_ties(R);
    if (!(m > 0)) { print_zero(); return; }
    std::printf("%a", std::log(m));
    for (int k = 0; k < nm; ++k) std::printf(" %d", code[rec[1 + k]]);
    std::printf("\n");
}

// ------------------------------------------------------------------------------------------------------------------------ draw
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

static void run_draw(const Network &net, int64_t b, const Query &q, uint32_t k0, uint32_t k1, FILE *fc, FILE *fm) {
    const int n = net.n_vars;
    const std::vector<int32_t> &card = net.card;
    std::vector<int32_t> row(n);
    auto write_none = [&]() {  // zero mass: -1 for every non-evidence variable
        for (int v = 0; v < n; ++v) row[v] = -1;
        for (size_t i = 0; i < q.ev.size(); ++i) row[q.ev[i]] = q.ec[i];
        const double one = 1.0;
        for (int64_t s = 0; s < q.n_samples; ++s) {
            std::fwrite(row.data(), 4, (size_t)n, fc);
            if (fm) std::fwrite(&one, 8, 1, fm);
        }
    };
    if (q.out_of_domain(net)) {
        write_none();
        std::printf("%a 0 0 0 0 %a 0\n", 0.0, 1.0);
        return;
    }
    const Request rq = q.request(ProgramKind::Draw);
    const std::string ve = validate_mpe_request(net, rq);
    if (!ve.empty()) fail(b, ve);
    Run R(net, b, rq, q);
    const PlanStats &st = R.st;
    if (st.kept_cells != st.arena_cells) fail(b, "kept_cells " + std::to_string(st.kept_cells) + " != arena_cells " + std::to_string(st.arena_cells));
    const uint32_t n_steps = R.n_steps();
    int n_elim = 0;
    R.run_steps(net, [&](uint32_t s, const GenericStep &g) {
        const bool fin = g.flags & kFlagFinal;
        if (g.flags & kFlagMax) fail(b, "step " + std::to_string(s) + " carries the MAX flag");
        if (fin != (s + 1 == n_steps)) fail(b, "the FINAL step is not the last one");
        if (fin && !(g.flags & kFlagRaw)) fail(b, "FINAL step without the RAW flag");
        if (fin && g.cx > 1) fail(b, "FINAL step eliminates a variable");
        if (g.cx > 1) ++n_elim;
        if (!fin)
            for (const Run::Table &t : R.tabs)
                if (g.out_off < t.off + t.cells && t.off < g.out_off + g.cells) fail(b, "the output of step " + std::to_string(s) + " overlaps a kept table");
        one_cell_final(b, g);
    });
    if (n_steps && R.final_.empty()) fail(b, "no FINAL step");
    const double mass = R.mass(1.0);
    // the record
    const uint32_t *rec = R.record();
    const uint32_t n_back = rec[0], n_fwd = rec[1], n_ev = rec[2];
    if ((int)n_back != n_elim) fail(b, "draw record has " + std::to_string(n_back) + " backward entries for " + std::to_string(n_elim) + " elimination steps");
    if (n_ev != q.ev.size()) fail(b, "draw record names " + std::to_string(n_ev) + " evidence variables");
    rec += 3;
    std::vector<char> known(n, 0);
    for (int v = 0; v < n; ++v) known[v] = card[v] <= 1;
    for (uint32_t i = 0; i < n_ev; ++i) known[rec[2 * i]] = 1;
    const uint32_t *ev_rec = rec;
    rec += 2 * n_ev;
    {   // every variable a draw reads is evidence or drawn before; every variable ends up drawn
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
        return;
    }
    double min_margin = 1.0;
    std::vector<uint64_t> low;
    std::vector<double> wv;
    for (int64_t s = 0; s < q.n_samples; ++s) {
        const uint64_t g = q.g_first + (uint64_t)s;
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
                    const double p = (in_off & kConstFlag) ? net.pool[(size_t)((in_off & ~kConstFlag) + ii)] : R.at((int64_t)in_off + ii);
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

// -------------------------------------------------------------------------------------------------------------------------- ev
static void run_ev(const Network &net, int64_t b, const Query &q, const std::string &mode) {
    Request rq = q.request(ProgramKind::Sum);
    if (mode == "reject") {
        const std::string ve = validate_request(net, rq);
        std::printf("%s\n", ve.empty() ? "ok" : ve.c_str());
        return;
    }
    rq.kind = ProgramKind::Raw;
    const std::string ve = validate_request(net, rq);
    if (!ve.empty()) fail(b, ve);
    int64_t qcells = 1;
    for (int32_t v : q.qv) qcells *= net.card[v];
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
        return;
    }
    std::vector<double> result((size_t)qcells, 0.0);
    if (!q.out_of_domain(net)) {
        Run R(net, b, rq, q);
        const uint32_t n_steps = R.n_steps();
        if (!n_steps) fail(b, "empty program");
        R.run_steps(net, [&](uint32_t s, const GenericStep &g) {
            const bool fin = g.flags & kFlagFinal, raw = g.flags & kFlagRaw;
            if (fin != (s + 1 == n_steps)) fail(b, "FINAL flag on step " + std::to_string(s) + " of " + std::to_string(n_steps));
            if (raw != fin) fail(b, "RAW flag on step " + std::to_string(s) + " does not match its FINAL flag");
            if (g.flags & kFlagMax) fail(b, "MAX flag in a sum program");
            if (fin && (g.cells != qcells || g.out_off != 0)) fail(b, "FINAL step of " + std::to_string(g.cells) + " cells at " + std::to_string(g.out_off));
        });
        result = R.final_;
    }
    for (int64_t c = 0; c < qcells; ++c) std::printf(c ? " %a" : "%a", result[(size_t)c]);
    std::printf("\n");
}

int main(int argc, char **argv) {
#ifdef PROG_SIM_KIND  // tools/{max,map,draw,ev}_sim.cpp: the command line of a former stand-alone twin, its kind fixed at build time
    static char fixed_kind[] = PROG_SIM_KIND;
    std::vector<char *> args{argv[0], fixed_kind};
    args.insert(args.end(), argv + 1, argv + argc);
    argc = (int)args.size();
    argv = args.data();
#endif
    // the options, taken out of the command line: what stays is the command line of before
    struct { long small_cells = -1, big_iters = -1, tile_h = -1, order_effort = -1; double second_above = -1, minfill_above = -1; const char *hints = nullptr, *lh = nullptr; } opt;
    std::vector<char *> pos;
    for (int i = 0; i < argc; ++i) {
        const std::string a = argv[i];
        if (i > 0 && a == "--ties") { g_report_ties = true; continue; }
        if (i > 0 && a == "--dump") { g_dump = true; continue; }
        if (i > 0 && a.rfind("--", 0) == 0) {
            if (i + 1 >= argc) { std::fprintf(stderr, "option %s without a value\n", argv[i]); return 2; }
            const char *v = argv[++i];
            if (a == "--small_cells") opt.small_cells = std::strtol(v, nullptr, 10);
            else if (a == "--big_iters") opt.big_iters = std::strtol(v, nullptr, 10);
            else if (a == "--tile_h") opt.tile_h = std::strtol(v, nullptr, 10);
            else if (a == "--order_effort") opt.order_effort = std::strtol(v, nullptr, 10);
            else if (a == "--second_above") opt.second_above = std::strtod(v, nullptr);
            else if (a == "--minfill_above") opt.minfill_above = std::strtod(v, nullptr);
            else if (a == "--hints") opt.hints = v;
            else if (a == "--lh") opt.lh = v;
            else { std::fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
            continue;
        }
        pos.push_back(argv[i]);
    }
    argc = (int)pos.size();
    argv = pos.data();
    const std::string kind_name = argc > 1 ? argv[1] : "";
    const bool is_ev = kind_name == "ev", is_draw = kind_name == "draw";
    if (!(kind_name == "max" || kind_name == "map" || is_draw || is_ev) || argc < (is_ev || is_draw ? 4 : 3)) {
        std::fprintf(stderr, "usage: prog_sim max net.txt | map net.txt | draw net.txt codes.bin [margins.bin] | ev run|compare|reject net.txt\n"
                             "       [--small_cells N] [--big_iters N] [--tile_h N] [--order_effort N] [--second_above X] [--minfill_above X] [--hints FILE] [--ties] [--lh FILE] [--dump]\n");
        return 2;
    }
    const Kind kind = is_ev ? Kind::Ev : is_draw ? Kind::Draw : kind_name == "map" ? Kind::Map : Kind::Max;
    const std::string mode = is_ev ? argv[2] : "";
    if (is_ev && mode != "run" && mode != "compare" && mode != "reject") { std::fprintf(stderr, "unknown mode %s\n", argv[2]); return 2; }
    if (opt.lh && (is_draw || (is_ev && mode != "run"))) { std::fprintf(stderr, "--lh: max, map and ev run only\n"); return 2; }
    slurp(argv[is_ev ? 3 : 2]);
    FILE *fc = nullptr, *fm = nullptr;
    if (is_draw) {
        fc = std::fopen(argv[3], "wb");
        if (!fc) { std::perror(argv[3]); return 2; }
        fm = argc > 4 ? std::fopen(argv[4], "wb") : nullptr;
        if (argc > 4 && !fm) { std::perror(argv[4]); return 2; }
    }
    Network net;
    read_network(net);
    if (opt.small_cells >= 0) net.small_cells = (int)opt.small_cells;
    if (opt.big_iters >= 0) net.big_iters = opt.big_iters;
    if (opt.tile_h >= 0) net.tile_h = (int)opt.tile_h;
    if (opt.order_effort >= 0) net.order_effort = (int)opt.order_effort;
    if (opt.second_above >= 0) net.second_above = opt.second_above;
    if (opt.minfill_above >= 0) net.minfill_above = opt.minfill_above;
    if (opt.hints) {
        FILE *fh = std::fopen(opt.hints, "rb");
        if (!fh) { std::perror(opt.hints); return 2; }
        long n_hints = 0, v = 0;
        std::vector<int32_t> pri;
        if (std::fscanf(fh, "%ld", &n_hints) != 1 || n_hints < 0) { std::fprintf(stderr, "%s: no hint count\n", opt.hints); return 2; }
        while (std::fscanf(fh, "%ld", &v) == 1) pri.push_back((int32_t)v);
        std::fclose(fh);
        if ((long)pri.size() != n_hints * net.n_vars) { std::fprintf(stderr, "%s: %zu priorities for %ld hints of %d variables\n", opt.hints, pri.size(), n_hints, net.n_vars); return 2; }
        net.set_hints((int32_t)n_hints, pri.data());
    }
    uint64_t seed = 0;
    bool no_prune = false;
    if (is_draw) { seed = getu(); no_prune = geti() == 0; }
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32) ^ 0x85EBCA6Bu;  // (the key of mibn_sample)
    const int64_t B = geti();
    // --lh: the findings of every request, read whole before the first request runs
    std::vector<std::vector<int32_t>> lh_vars((size_t)B);
    std::vector<std::vector<std::vector<double>>> lh_w((size_t)B);
    if (opt.lh) {
        FILE *fl = std::fopen(opt.lh, "rb");
        if (!fl) { std::perror(opt.lh); return 2; }
        char tok[128];
        auto word = [&]() -> const char * {
            if (std::fscanf(fl, "%127s", tok) != 1) { std::fprintf(stderr, "%s ends early\n", opt.lh); std::exit(2); }
            return tok;
        };
        for (int64_t b = 0; b < B; ++b) {
            const long k = std::strtol(word(), nullptr, 10);
            for (long i = 0; i < k; ++i) {
                const long v = std::strtol(word(), nullptr, 10);
                if (v < 0 || v >= net.n_vars) { std::fprintf(stderr, "%s: request %lld names variable %ld\n", opt.lh, (long long)b, v); return 2; }
                lh_vars[(size_t)b].push_back((int32_t)v);
                lh_w[(size_t)b].emplace_back();
                for (int c = 0; c < net.card[v]; ++c) lh_w[(size_t)b].back().push_back(std::strtod(word(), nullptr));
            }
        }
        std::fclose(fl);
    }
    for (int64_t b = 0; b < B; ++b) {
        Query q(kind, no_prune);
        q.lv = lh_vars[(size_t)b];
        q.lw = lh_w[(size_t)b];
        switch (kind) {
            case Kind::Max: run_max(net, b, q); break;
            case Kind::Map: run_map(net, b, q); break;
            case Kind::Draw: run_draw(net, b, q, k0, k1, fc, fm); break;
            case Kind::Ev: run_ev(net, b, q, mode); break;
        }
    }
    if (fc) std::fclose(fc);
    if (fm) std::fclose(fm);
    return 0;
}
