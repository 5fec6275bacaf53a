// Host twin of the sampling family's launch planning: sorobn_amd/csrc/sampler_plan.h (the header gibbs_run and sample_run include)
// on a CPU, linked against planner.cpp.  Prints what a call would launch - nothing is computed.
//
//   g++ -O2 -std=c++17 tools/sampler_plan_sim.cpp sorobn_amd/csrc/planner.cpp -lpthread -o sampler_plan_sim
//   sampler_plan_sim < input
//
// input: the network prefix of prog_sim (n_vars, card, scope_off, scope_vars, value_off, values), then one command per line:
//   gibbs   lds_mode n_chains cond_var  n_q q..  n_e e.. codes..  n_cycle cycle..       (n_cycle -1: no caller's cycle)
//   sample  mode n_samples cdf_stride  n_q q..  n_clamp v.. codes..  n_ev v.. codes..
//   glayout n_vars hist_cells pool_cells fast prog_words
//   slayout n_vars hist_cells
// output: one line of key=value pairs per command (lists comma separated; vars = the eight words of every GibbsVar), or
//   error=<MIBN_* code> msg=<the message, to the end of the line>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../sorobn_amd/csrc/sampler_plan.h"

using namespace mibn;

static int64_t geti() {
    long long v;
    if (!(std::cin >> v)) { std::fprintf(stderr, "input ends early\n"); std::exit(2); }
    return v;
}
static std::vector<int32_t> getv(int64_t n) {
    std::vector<int32_t> a((size_t)std::max<int64_t>(0, n));
    for (auto &x : a) x = (int32_t)geti();
    return a;
}
static void put_list(const char *key, const int32_t *a, size_t n) {
    std::printf(" %s=", key);
    for (size_t i = 0; i < n; ++i) std::printf(i ? ",%d" : "%d", a[i]);
}
static void put_pack(const SamplerPack &P) {
    put_list("vars", &P.vars.data()->card, P.vars.size() * 8);
    put_list("pack", P.words.data(), P.words.size());
    std::printf("\n");
}

int main() {
    Network net;
    {
        const int n = (int)geti();
        std::vector<int32_t> card = getv(n);
        std::vector<int64_t> scope_off((size_t)n + 1), value_off((size_t)n + 1);
        for (auto &o : scope_off) o = geti();
        std::vector<int32_t> scope_vars = getv(scope_off[n]);
        for (auto &o : value_off) o = geti();
        std::vector<double> values((size_t)value_off[n]);
        std::string tok;
        for (auto &v : values) { std::cin >> tok; v = std::strtod(tok.c_str(), nullptr); }
        const std::string e = net.set(n, card.data(), scope_off.data(), scope_vars.data(), value_off.data(), values.data());
        if (!e.empty()) { std::fprintf(stderr, "set: %s\n", e.c_str()); return 2; }
    }
    std::string cmd, err;
    while (std::cin >> cmd) {
        if (cmd == "glayout") {
            const size_t n = (size_t)geti(), cells = (size_t)geti(), pool = (size_t)geti();
            const bool fast = geti() != 0;
            const GibbsLayout<size_t> L = gibbs_layout<size_t>(n, cells, pool, fast, (size_t)geti());
            std::printf("hist=%zu pool=%zu prog=%zu total=%zu\n", L.hist, L.pool, L.prog, L.total);
        } else if (cmd == "slayout") {
            const size_t n = (size_t)geti();
            const SampleLayout<size_t> L = sample_layout<size_t>(n, (size_t)geti());
            std::printf("hsum=%zu hcnt=%zu total=%zu\n", L.hsum, L.hcnt, L.total);
        } else if (cmd == "gibbs") {
            const int lds_mode = (int)geti();
            const int64_t n_chains = geti();
            const int32_t cond_var = (int32_t)geti();
            const std::vector<int32_t> q = getv(geti());
            const int64_t n_e = geti();
            const std::vector<int32_t> ev = getv(n_e), ec = getv(n_e);
            const int64_t n_cycle = geti();
            const std::vector<int32_t> cycle = getv(n_cycle);
            GibbsPlan G;
            const int rc = gibbs_plan(net, lds_mode, (int32_t)q.size(), q.data(), (int32_t)n_e, ev.data(), ec.data(), n_cycle < 0 ? nullptr : cycle.data(),
                                      n_chains, cond_var, G, err);
            if (rc) { std::printf("error=%d msg=%s\n", rc, err.c_str()); continue; }
            std::printf("form=%s hist=%zu pool=%zu prog=%zu total=%zu blocks=%u n_cycle=%d hist_cells=%d pool_cells=%d uprog_words=%d prog_words=%d cond_pos=%d",
                        gibbs_form_name(G.form), G.lds.hist, G.lds.pool, G.lds.prog, G.lds.total, G.blocks, G.n_cycle, G.hist_cells, G.pool_cells,
                        G.uprog_words, G.prog_words, G.cond_pos);
            std::printf(" o_sv=%zu o_ss=%zu o_ch=%zu o_cy=%zu o_q=%zu o_qs=%zu o_up=%zu o_uo=%zu", G.o_sv, G.o_ss, G.o_ch, G.o_cy, G.o_q, G.o_qs, G.o_up, G.o_uo);
            put_pack(G.pack);
        } else if (cmd == "sample") {
            const int mode = (int)geti();
            const int64_t n_samples = geti();
            const int32_t cdf_stride = (int32_t)geti();
            const std::vector<int32_t> q = getv(geti());
            const int64_t n_c = geti();
            const std::vector<int32_t> cv = getv(n_c), cc = getv(n_c);
            const int64_t n_e = geti();
            const std::vector<int32_t> ev = getv(n_e), ec = getv(n_e);
            SamplePlan S;
            const int rc = sample_plan(net, mode, (int32_t)q.size(), q.data(), (int32_t)n_c, cv.data(), cc.data(), (int32_t)n_e, ev.data(), ec.data(), n_samples,
                                       cdf_stride, S, err);
            if (rc) { std::printf("error=%d msg=%s\n", rc, err.c_str()); continue; }
            std::printf("hsum=%zu hcnt=%zu total=%zu blocks=%u cells=%lld hist_cells=%d out_bytes=%zu probe_states=%zu o_sv=%zu o_ss=%zu o_q=%zu o_qs=%zu o_ev=%zu o_ec=%zu",
                        S.lds.hsum, S.lds.hcnt, S.lds.total, S.blocks, (long long)S.cells, S.hist_cells, S.out_bytes, S.probe_states, S.o_sv, S.o_ss, S.o_q,
                        S.o_qs, S.o_ev, S.o_ec);
            put_pack(S.pack);
        } else {
            std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
