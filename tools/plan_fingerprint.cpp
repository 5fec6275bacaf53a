// Regression guard for planner optimisations (CPU only): plans seeded random requests on a family of synthetic networks -
// uniform and mixed cardinalities, grids and random DAGs, every option set the tests force - and prints one fingerprint of the
// emitted programs + work items + statistics per (network, option set).  A change that is meant to make the planner faster must
// not move a single line of this output.
// A second section pins the flavours only the host plans - max, unnormalised (raw), draw and map programs, pruned and not - on
// eight of these networks and a star: program words with their records, the empty records of skipped requests, per-request costs,
// arena needs, argmax / kept cells, and the schedule.
// A third section pins how the engine cuts every schedule of the first section into kernel launches (planner.h level_groups): per
// network and per setting of the four options that route a class to a kernel, one hash over the launch groups of the network's six
// schedules - route, level, statistics class, workgroup ranges, grid, bytes (bit pattern) and the range of Launch entries.
//   plan_fingerprint [B [B2]]   B requests per pair of the first and third section (default 1500), B2 of the second (200); 0 skips them
//   g++ -O2 -mpopcnt -std=c++17 tools/plan_fingerprint.cpp sorobn_amd/csrc/planner.cpp -lpthread -o /tmp/plan_fingerprint
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../sorobn_amd/csrc/planner.h"
using namespace mibn;

struct Spec {
    std::string name;
    std::vector<int32_t> card, scope_vars;
    std::vector<int64_t> scope_off{0}, value_off{0};
    std::vector<double> values;
    void add(const std::vector<int32_t> &parents, int v) {
        int64_t cells = card[v];
        for (int p : parents) { scope_vars.push_back(p); cells *= card[p]; }
        scope_vars.push_back(v);
        scope_off.push_back((int64_t)scope_vars.size());
        for (int64_t i = 0; i < cells; ++i) values.push_back(0.25 + 0.5 * ((i * 2654435761u) % 97) / 97.0);
        value_off.push_back((int64_t)values.size());
    }
};

static Spec grid(int R, int C, const std::vector<int> &cards, uint64_t seed, const char *name) {
    Spec s;
    s.name = name;
    std::mt19937_64 rng(seed);
    for (int v = 0; v < R * C; ++v) s.card.push_back(cards[rng() % cards.size()]);
    for (int v = 0; v < R * C; ++v) {
        std::vector<int32_t> pa;
        if (v / C) pa.push_back(v - C);
        if (v % C) pa.push_back(v - 1);
        s.add(pa, v);
    }
    return s;
}

static Spec random_dag(int n, int max_parents, const std::vector<int> &cards, uint64_t seed, const char *name) {
    Spec s;
    s.name = name;
    std::mt19937_64 rng(seed);
    for (int v = 0; v < n; ++v) s.card.push_back(cards[rng() % cards.size()]);
    for (int v = 0; v < n; ++v) {
        std::vector<int32_t> pa;
        const int np = v ? (int)(rng() % (std::min(v, max_parents) + 1)) : 0;
        while ((int)pa.size() < np) {
            const int p = (int)(rng() % v);
            // mostly recent nodes: long chains of interaction, like a layered network
            const int q = v - 1 - (int)(rng() % std::min(v, 12));
            const int pick = (rng() & 3) ? q : p;
            if (std::find(pa.begin(), pa.end(), pick) == pa.end()) pa.push_back(pick);
        }
        std::sort(pa.begin(), pa.end());
        s.add(pa, v);
    }
    return s;
}

static Spec star(int children, const std::vector<int> &cards, uint64_t seed, const char *name) {
    // one root, every other variable its child: eliminating the root joins children + 1 tables, more than kMaxIn
    Spec s;
    s.name = name;
    std::mt19937_64 rng(seed);
    for (int v = 0; v <= children; ++v) s.card.push_back(cards[rng() % cards.size()]);
    s.add({}, 0);
    for (int v = 1; v <= children; ++v) s.add({0}, v);
    return s;
}

struct Opt {
    const char *name;
    int small_cells;
    int64_t big_iters;
    double minfill_above;
    int fuse, chain, sweep, sweep_min, outer, prune, order_weights;
};

static uint64_t fnv(uint64_t h, const void *p, size_t n) {
    const unsigned char *c = (const unsigned char *)p;
    for (size_t i = 0; i < n; ++i) h = (h ^ c[i]) * 1099511628211ull;
    return h;
}

// The programs only the host plans.  max and draw take no query variables; map's are the MAP variables.
struct Flavour {
    const char *name;
    ProgramKind kind;
    bool no_prune;
};

static void host_flavours(const std::vector<Spec> &specs, int64_t nb) {
    const Flavour flavours[] = {
        {"max", ProgramKind::Max, false},   {"raw", ProgramKind::Raw, false},        {"raw_noprune", ProgramKind::Raw, true},
        {"draw_noprune", ProgramKind::Draw, true}, {"draw", ProgramKind::Draw, false}, {"map_noprune", ProgramKind::Map, true},
        {"map", ProgramKind::Map, false},
    };
    for (const Spec &s : specs) {
        const int n = (int)s.card.size();
        for (const Flavour &f : flavours) {
            Network net;
            std::string e = net.set(n, s.card.data(), s.scope_off.data(), s.scope_vars.data(), s.value_off.data(), s.values.data());
            if (!e.empty()) { std::printf("%s: %s\n", s.name.c_str(), e.c_str()); std::exit(1); }
            net.plan_cache = 0;
            const bool takes_query = f.kind == ProgramKind::Raw || f.kind == ProgramKind::Map;
            std::mt19937_64 rng(4321);
            std::vector<int64_t> q_off{0}, e_off{0}, out_off{0};
            std::vector<int32_t> qv, ev, ec;
            std::vector<char> skip((size_t)nb, 0);
            for (int64_t b = 0; b < nb; ++b) {
                skip[(size_t)b] = b % 16 == 15;  // (their evidence is kept: the empty record of the flavour carries it)
                // 0 to 4 evidence variables, drawn one by one; a quarter of the requests has 8 more, and theirs are a run of consecutive
                // ids from a random start: whole CPTs become scalars there (a grid's first row), so that the final product joins more
                // than kMaxIn tables on every network
                const int nq_drawn = (int)(rng() % 5), ne_drawn = (int)(rng() % 5);
                const bool run = rng() % 4 == 0;
                const int ne = std::min(n, ne_drawn + (run ? 8 : 0)), nq = takes_query ? std::min(n - ne, nq_drawn) : 0;
                std::vector<int> pick;
                const int start = (int)(rng() % n);
                while ((int)pick.size() < ne) {
                    const int v = run ? (start + (int)pick.size()) % n : (int)(rng() % n);
                    if (std::find(pick.begin(), pick.end(), v) == pick.end()) pick.push_back(v);
                }
                while ((int)pick.size() < ne + nq) {
                    const int v = (int)(rng() % n);
                    if (std::find(pick.begin(), pick.end(), v) == pick.end()) pick.push_back(v);
                }
                int64_t cells = 1;
                for (int i = 0; i < (int)pick.size(); ++i) {
                    if (i < ne) { ev.push_back(pick[i]); ec.push_back((int)(rng() % s.card[pick[i]])); }
                    else { qv.push_back(pick[i]); if (f.kind == ProgramKind::Raw) cells *= s.card[pick[i]]; }
                }
                q_off.push_back((int64_t)qv.size());
                e_off.push_back((int64_t)ev.size());
                out_off.push_back(out_off.back() + cells);
            }
            if (qv.empty()) qv.push_back(0);
            if (ev.empty()) { ev.push_back(0); ec.push_back(0); }
            ThreadPool pool(1);
            std::vector<ProgBuf> bufs;
            BatchPlan bp;
            plan_batch(net, pool, bufs, 0, nb, q_off.data(), qv.data(), e_off.data(), ev.data(), ec.data(), out_off.data(), skip.data(), bp,
                       f.no_prune, nullptr, nullptr, -1, f.kind);
            uint64_t h = 1469598103934665603ull;
            int64_t product_only = 0;
            if (!bp.err.empty()) {
                h = fnv(h, bp.err.data(), bp.err.size());
            } else {
                h = fnv(h, bufs[0].data, bufs[0].size * 4);
                for (const Tag &t : bp.tags[0]) {
                    h = fnv(h, &t.rel_off, 4); h = fnv(h, &t.a, 4); h = fnv(h, &t.wgs, 4); h = fnv(h, &t.level, 2); h = fnv(h, &t.kid, 2);
                    h = fnv(h, &t.bytes, 4);
                }
                h = fnv(h, bp.cost.data(), bp.cost.size() * 8);
                h = fnv(h, bp.arena_need.data(), bp.arena_need.size() * 8);
                h = fnv(h, &bp.st.alg_flops, 8);
                h = fnv(h, &bp.st.n_steps, 8);
                Schedule sc;
                build_schedule(net, bp, bufs, 0, nb, sc);
                h = fnv(h, sc.items.data(), sc.items.size() * sizeof(Item));
                h = fnv(h, sc.wg_item.data(), sc.wg_item.size() * 4);
                h = fnv(h, sc.arena_off.data(), sc.arena_off.size() * 8);
                std::vector<uint32_t> one;
                for (int64_t b = 0; b < nb; ++b) {
                    const uint32_t *p = bufs[0].data + bp.local_off[(size_t)b];
                    for (uint32_t k = 0, off = 1; k < p[0]; ++k, off += p[off + 6])  // steps with cx = 1 that are not FINAL
                        product_only += (p[off + 1] & 0xffffu) == 1 && !((p[off + 1] >> 16) & kFlagFinal);
                    if (skip[(size_t)b]) continue;
                    // the same request through plan_request: the same words, and the cells nothing else reports
                    Request rq;
                    rq.nq = (int32_t)(q_off[b + 1] - q_off[b]); rq.qvars = qv.data() + q_off[b];
                    rq.ne = (int32_t)(e_off[b + 1] - e_off[b]); rq.evars = ev.data() + e_off[b]; rq.ecodes = ec.data() + e_off[b];
                    rq.out_off = out_off[b];
                    rq.no_prune = f.no_prune;
                    rq.kind = f.kind;
                    PlanStats st;
                    one.clear();
                    e = plan_request(net, rq, one, st);
                    const size_t words = (size_t)((b + 1 < nb ? bp.local_off[(size_t)b + 1] : bufs[0].size) - bp.local_off[(size_t)b]);
                    if (!e.empty() || one.size() != words || std::memcmp(one.data(), p, words * 4)) {
                        std::printf("%s %s: plan_request and plan_batch disagree on request %lld %s\n", s.name.c_str(), f.name, (long long)b, e.c_str());
                        std::exit(1);
                    }
                    h = fnv(h, &st.argmax_cells, 8);
                    h = fnv(h, &st.kept_cells, 8);
                }
            }
            std::printf("%-16s %-18s %016llx  words %zu steps %.0f bytes %.6g product-only %lld%s\n", s.name.c_str(), f.name,
                        (unsigned long long)h, bp.total_words, bp.st.n_steps, bp.st.alg_bytes, (long long)product_only,
                        bp.err.empty() ? "" : (" ERR " + bp.err).c_str());
            for (auto &b : bufs) b.release();
        }
    }
}

// third section: the launch groups of one schedule into the 16 hashes of its network, one per LevelRouteOpts setting
static LevelRouteOpts route_setting(int k) { return {(k & 1) != 0, (k & 2) != 0, (k & 4) != 0, (k & 8) != 0}; }
static void hash_groups(const Schedule &sc, uint64_t *h16) {
    std::vector<LaunchGroup> groups;
    for (int k = 0; k < 16; ++k) {
        level_groups(sc, route_setting(k), groups);
        uint64_t h = h16[k];
        for (const LaunchGroup &g : groups) {  // (field by field: the struct has padding)
            const int route = (int)g.route;
            h = fnv(h, &route, 4); h = fnv(h, &g.level, 4); h = fnv(h, &g.stat_kid, 4); h = fnv(h, &g.wg_level, 8); h = fnv(h, &g.wg_first, 8);
            h = fnv(h, &g.grid, 8); h = fnv(h, &g.alg_bytes, 8); h = fnv(h, &g.first_launch, 8); h = fnv(h, &g.n_launches, 8);
        }
        h16[k] = fnv(h, "|", 1);  // (a schedule ends here)
    }
}

int main(int argc, char **argv) {
    const int64_t B = argc > 1 ? atoll(argv[1]) : 1500, B2 = argc > 2 ? atoll(argv[2]) : 200;
    std::vector<Spec> specs;
    specs.push_back(grid(10, 10, {4}, 1, "grid10x10_k4"));
    specs.push_back(grid(5, 10, {8}, 2, "grid5x10_k8"));
    specs.push_back(grid(8, 8, {3}, 3, "grid8x8_k3"));
    specs.push_back(grid(9, 9, {2, 3, 4, 5}, 4, "grid9x9_mixed"));
    specs.push_back(grid(12, 10, {2, 4}, 5, "grid12x10_k24"));
    specs.push_back(grid(7, 18, {4}, 6, "grid7x18_k4"));
    specs.push_back(grid(6, 6, {1, 2, 4, 16}, 7, "grid6x6_k1_16"));
    specs.push_back(random_dag(40, 3, {2, 3, 4, 5}, 8, "dag40_mixed"));
    specs.push_back(random_dag(90, 3, {2, 3, 4}, 9, "dag90_mixed"));
    specs.push_back(random_dag(128, 2, {4}, 10, "dag128_k4"));
    specs.push_back(random_dag(160, 2, {2, 3}, 11, "dag160_k23"));  // > 128 variables: the generic bit sets
    specs.push_back(random_dag(12, 3, {2, 3, 4, 5, 17, 33}, 12, "dag12_wide"));
    const Opt opts[] = {
        {"default", 1024, 4096, 2e7, 1, 1, 5, 2, 1, 1, 1},
        {"minfill_always", 1024, 4096, 0.0, 1, 1, 5, 2, 1, 1, 1},
        {"forced_small", 4, 16, 0.0, 1, 1, 5, 2, 1, 1, 1},
        {"forced_16_64", 16, 64, 2e7, 1, 1, 5, 3, 1, 1, 1},
        {"no_fuse", 1024, 4096, 2e7, 0, 0, 0, 2, 0, 1, 0},
        {"no_sweep_noprune", 64, 256, 1e5, 1, 1, 0, 2, 1, 0, 1},
    };
    std::vector<uint64_t> route_hash(specs.size() * 16, 1469598103934665603ull);
    for (const Spec &s : specs) {
        if (B <= 0) break;
        const int n = (int)s.card.size();
        for (const Opt &o : opts) {
            Network net;
            std::string e = net.set(n, s.card.data(), s.scope_off.data(), s.scope_vars.data(), s.value_off.data(), s.values.data());
            if (!e.empty()) { std::printf("%s: %s\n", s.name.c_str(), e.c_str()); return 1; }
            net.small_cells = o.small_cells; net.big_iters = o.big_iters; net.minfill_above = o.minfill_above; net.fuse = o.fuse;
            net.chain = o.chain; net.sweep = o.sweep; net.sweep_min = o.sweep_min; net.outer = o.outer; net.prune = o.prune;
            net.order_weights = o.order_weights;
            net.plan_cache = 0;
            std::vector<int32_t> hint(n);
            for (int v = 0; v < n; ++v) hint[v] = v;
            net.set_hints(1, hint.data());
            std::mt19937_64 rng(1234);
            std::vector<int64_t> q_off{0}, e_off{0}, out_off{0};
            std::vector<int32_t> qv, ev, ec;
            const bool heavy = !o.prune || n > 128;
            const int64_t nb = heavy ? std::max<int64_t>(B / 8, 16) : B;
            for (int64_t b = 0; b < nb; ++b) {
                const int nq = 1 + (int)(rng() % 3 == 0) + (int)(rng() % 7 == 0);
                const int ne = (int)(rng() % 5) + (rng() % 4 == 0 ? 8 : 0);
                std::vector<int> pick;
                while ((int)pick.size() < std::min(n, nq + ne)) {
                    const int v = (int)(rng() % n);
                    if (std::find(pick.begin(), pick.end(), v) == pick.end()) pick.push_back(v);
                }
                int64_t cells = 1;
                for (int i = 0; i < (int)pick.size(); ++i) {
                    if (i < nq) { qv.push_back(pick[i]); cells *= s.card[pick[i]]; }
                    else { ev.push_back(pick[i]); ec.push_back((int)(rng() % s.card[pick[i]])); }
                }
                q_off.push_back((int64_t)qv.size());
                e_off.push_back((int64_t)ev.size());
                out_off.push_back(out_off.back() + cells);
            }
            ThreadPool pool(1);
            std::vector<ProgBuf> bufs;
            BatchPlan bp;
            if (ev.empty()) { ev.push_back(0); ec.push_back(0); }
            plan_batch(net, pool, bufs, 0, nb, q_off.data(), qv.data(), e_off.data(), ev.data(), ec.data(), out_off.data(), nullptr, bp,
                       !o.prune);
            uint64_t h = 1469598103934665603ull;
            if (!bp.err.empty()) {
                h = fnv(h, bp.err.data(), bp.err.size());
            } else {
                h = fnv(h, bufs[0].data, bufs[0].size * 4);
                for (const Tag &t : bp.tags[0]) {  // (field by field: the struct has padding)
                    h = fnv(h, &t.rel_off, 4); h = fnv(h, &t.a, 4); h = fnv(h, &t.wgs, 4); h = fnv(h, &t.level, 2); h = fnv(h, &t.kid, 2);
                    h = fnv(h, &t.bytes, 4);
                }
                h = fnv(h, bp.cost.data(), bp.cost.size() * 8);
                h = fnv(h, bp.arena_need.data(), bp.arena_need.size() * 8);
                h = fnv(h, &bp.st.alg_flops, 8);
                h = fnv(h, &bp.st.n_steps, 8);
                Schedule sc;
                build_schedule(net, bp, bufs, 0, nb, sc);
                h = fnv(h, sc.items.data(), sc.items.size() * sizeof(Item));
                h = fnv(h, sc.wg_item.data(), sc.wg_item.size() * 4);
                h = fnv(h, sc.arena_off.data(), sc.arena_off.size() * 8);
                hash_groups(sc, route_hash.data() + (size_t)(&s - specs.data()) * 16);
            }
            std::printf("%-16s %-18s %016llx  words %zu steps %.0f bytes %.6g%s\n", s.name.c_str(), o.name, (unsigned long long)h,
                        bp.total_words, bp.st.n_steps, bp.st.alg_bytes, bp.err.empty() ? "" : (" ERR " + bp.err).c_str());
            for (auto &b : bufs) b.release();
        }
    }
    if (B2 > 0) {
        std::vector<Spec> host;
        for (const char *name : {"grid10x10_k4", "grid8x8_k3", "grid9x9_mixed", "grid6x6_k1_16", "dag40_mixed", "dag90_mixed", "dag160_k23", "dag12_wide"})
            host.push_back(*std::find_if(specs.begin(), specs.end(), [&](const Spec &s) { return s.name == name; }));
        host.push_back(star(9, {2, 3, 4}, 13, "star10"));
        host_flavours(host, B2);
    }
    for (size_t i = 0; B > 0 && i < specs.size(); ++i)
        for (int k = 0; k < 16; ++k) {
            const LevelRouteOpts o = route_setting(k);
            std::printf("%-16s groups split_kinds=%d seg_kernel=%d mfma_kernel=%d sweep_dma=%d  %016llx\n", specs[i].name.c_str(), (int)o.split_kinds,
                        (int)o.seg_kernel, (int)o.mfma_kernel, (int)o.sweep_dma, (unsigned long long)route_hash[i * 16 + (size_t)k]);
        }
    return 0;
}
