// Host twin of loopy belief propagation's launch planning: sorobn_amd/csrc/bp_plan.h (the header bp_kernel.hip.h and mibn_bp_batch
// include) on a CPU, linked against planner.cpp.  Prints what a call would launch - nothing is computed.
//
//   g++ -O2 -std=c++17 tools/bp_plan_sim.cpp sorobn_amd/csrc/planner.cpp -lpthread -o bp_plan_sim
//   bp_plan_sim < input
//
// input: the network prefix of prog_sim (n_vars, card, scope_off, scope_vars, value_off, values), then one command per line:
//   plan    lds_mode                              the records, offsets, layout and form of a call under option bp_lds = lds_mode
//   layout  cells lam_cells                       bp_layout alone
//   launch  lds_mode chunk budget_bytes           requests of one launch (0: a slab does not fit)
//   args    max_iterations tol damping            the argument check (tol and damping as strtod reads them: nan, -1, 0x1p-3 ..)
//   mpe     lds_mode                              mibn_bp_mpe_batch: the colouring (colour of each variable, members per colour as CSR), bp_mpe_layout, the form
//   mpe_args max_iterations tol damping polish    its argument check
//   ev      lds_mode                              mibn_bp_evidence_batch: bp_ev_layout, the form, the family-belief row (fcells, foff)
//   ev_launch lds_mode rows chunk budget_bytes    its requests of one launch (rows != 0: with the family-belief buffer; 0: one does not fit)
//   ev_acc  lds_mode n_acc B w_0 .. w_(B-1)       its check of n_acc (negative: no acc) and of the weights (B = 0: weight NULL)
// output: one line of key=value pairs per command (lists comma separated; edges / vars = the eight words of every record), or
//   error=<MIBN_* code> msg=<the message, to the end of the line>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../sorobn_amd/csrc/bp_plan.h"

using namespace mibn;

static int64_t geti() {
    long long v;
    if (!(std::cin >> v)) { std::fprintf(stderr, "input ends early\n"); std::exit(2); }
    return v;
}
static double getd() {
    std::string tok;
    if (!(std::cin >> tok)) { std::fprintf(stderr, "input ends early\n"); std::exit(2); }
    return std::strtod(tok.c_str(), nullptr);
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

int main() {
    Network net;
    {
        const int n = (int)geti();
        std::vector<int32_t> card = getv(n);
        std::vector<int64_t> scope_off((size_t)n + 1), value_off((size_t)n + 1);
        for (auto &o : scope_off) o = geti();
        std::vector<int32_t> scope_vars = getv(scope_off[(size_t)n]);
        for (auto &o : value_off) o = geti();
        std::vector<double> values((size_t)value_off[(size_t)n]);
        for (auto &v : values) v = getd();
        const std::string e = net.set(n, card.data(), scope_off.data(), scope_vars.data(), value_off.data(), values.data());
        if (!e.empty()) { std::fprintf(stderr, "set: %s\n", e.c_str()); return 2; }
    }
    std::string cmd, err;
    while (std::cin >> cmd) {
        if (cmd == "layout") {
            const size_t cells = (size_t)geti();
            const BpLayout<size_t> L = bp_layout<size_t>(cells, (size_t)geti());
            std::printf("mu0=%zu mu1=%zu nu=%zu lam=%zu red=%zu total=%zu\n", L.mu0, L.mu1, L.nu, L.lam, L.red, L.total);
        } else if (cmd == "args") {
            const int32_t it = (int32_t)geti();
            const double tol = getd(), damping = getd();
            const int rc = bp_check_args(it, tol, damping, err);
            if (rc) std::printf("error=%d msg=%s\n", rc, err.c_str());
            else std::printf("ok=1\n");
        } else if (cmd == "mpe") {
            const int lds_mode = (int)geti();
            BpMpePlan M;
            const int rc = bp_mpe_plan(net, lds_mode, M, err);
            if (rc) { std::printf("error=%d msg=%s\n", rc, err.c_str()); continue; }
            const BpMpeLayout<size_t> &L = M.lds;
            std::printf("form=%s n_colours=%d mu0=%zu mu1=%zu nu=%zu lam=%zu term=%zu part=%zu cur=%zu kept=%zu red=%zu total=%zu slab=%zu threads=%d",
                        bp_form_name(M.form), M.col.n_colours, L.mu0, L.mu1, L.nu, L.lam, L.term, L.part, L.cur, L.kept, L.red, L.total, M.slab_bytes,
                        M.bp.threads);
            put_list("colour", M.col.colour.data(), M.col.colour.size());
            put_list("col_off", M.col.off.data(), M.col.off.size());
            put_list("col_members", M.col.members.data(), M.col.members.size());
            std::printf("\n");
        } else if (cmd == "mpe_args") {
            const int32_t it = (int32_t)geti();
            const double tol = getd(), damping = getd();
            const int rc = bp_mpe_check_args(it, tol, damping, (int32_t)geti(), err);
            if (rc) std::printf("error=%d msg=%s\n", rc, err.c_str());
            else std::printf("ok=1\n");
        } else if (cmd == "ev" || cmd == "ev_launch" || cmd == "ev_acc") {
            const int lds_mode = (int)geti();
            BpEvPlan E;
            const int rc = bp_ev_plan(net, lds_mode, E, err);
            if (cmd == "ev_launch") {
                const bool rows = geti() != 0;
                const int64_t chunk = geti();
                const double budget = getd();
                if (rc) { std::printf("error=%d msg=%s\n", rc, err.c_str()); continue; }
                std::printf("requests=%lld\n", (long long)bp_ev_launch_requests(E, rows, chunk, budget));
                continue;
            }
            if (cmd == "ev_acc") {
                const int64_t n_acc = geti(), B = geti();  // n_acc < 0: no acc; then B weights (B = 0: weight NULL)
                std::vector<double> w((size_t)std::max<int64_t>(0, B));
                for (auto &x : w) x = getd();
                if (rc) { std::printf("error=%d msg=%s\n", rc, err.c_str()); continue; }
                const int rc2 = bp_ev_check_acc(E, n_acc >= 0, n_acc, B ? w.data() : nullptr, B, err);
                if (rc2) std::printf("error=%d msg=%s\n", rc2, err.c_str());
                else std::printf("ok=1\n");
                continue;
            }
            if (rc) { std::printf("error=%d msg=%s\n", rc, err.c_str()); continue; }
            const BpEvLayout<size_t> &L = E.lds;
            std::printf("form=%s fcells=%d mu0=%zu mu1=%zu nu=%zu lam=%zu zf=%zu term=%zu part=%zu red=%zu total=%zu slab=%zu threads=%d iter_bytes=%.0f",
                        bp_form_name(E.form), E.fcells, L.mu0, L.mu1, L.nu, L.lam, L.zf, L.term, L.part, L.red, L.total, E.slab_bytes, E.bp.threads,
                        E.bp.iter_bytes);
            put_list("foff", E.foff.data(), E.foff.size());
            std::printf("\n");
        } else if (cmd == "plan" || cmd == "launch") {
            const int lds_mode = (int)geti();
            BpPlan P;
            const int rc = bp_plan(net, lds_mode, P, err);
            if (cmd == "launch") {
                const int64_t chunk = geti();
                const double budget = getd();
                if (rc) { std::printf("error=%d msg=%s\n", rc, err.c_str()); continue; }
                std::printf("requests=%lld\n", (long long)bp_launch_requests(P, chunk, budget));
                continue;
            }
            if (rc) { std::printf("error=%d msg=%s\n", rc, err.c_str()); continue; }
            std::printf("form=%s n_edges=%zu cells=%d lam_cells=%d mu0=%zu mu1=%zu nu=%zu lam=%zu red=%zu total=%zu slab=%zu threads=%d iter_bytes=%.0f",
                        bp_form_name(P.form), P.edges.size(), P.cells, P.lam_cells, P.lds.mu0, P.lds.mu1, P.lds.nu, P.lds.lam, P.lds.red, P.lds.total,
                        P.slab_bytes, P.threads, P.iter_bytes);
            put_list("edges", &P.edges.data()->factor, P.edges.size() * 8);
            put_list("vars", &P.vars.data()->card, P.vars.size() * 8);
            put_list("nbr", P.nbr.data(), P.nbr.size());
            put_list("nbr_moff", P.nbr_moff.data(), P.nbr_moff.size());
            std::printf("\n");
        } else {
            std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
