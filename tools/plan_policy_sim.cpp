// Host twin of the adaptive planning policy (sorobn_amd/csrc/plan_policy.h): scripted sequences in, the decisions out.
//   g++ -O2 -std=c++17 tools/plan_policy_sim.cpp -o plan_policy_sim && ./plan_policy_sim < script
// One command per line; after each the whole state is printed as "key=value ..." (tests/test_plan_policy_host.py).
//   set <field> <value>                                  any field of PlanPolicy or of the knobs (gpu_emit, gpu_search, minfill_above)
//   start <call> <threads> <plan_ms> <kernel_ms> <requests> <order_net_ok> <emit_net_ok>
//   share <n> <whole> <wave>                             prints nd
//   chunk <n> <nd> <host_ms> <dev_ms> <chunk> <wave>
//   end <B> <call_fixed_ms>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "../sorobn_amd/csrc/plan_policy.h"

int main() {
    mibn::PlanPolicy p;
    mibn::PlanPolicy::Knobs k{0, 0, p.base_minfill};
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        long long nd = -1;
        int ruled = 0;
        if (cmd == "set") {
            std::string f;
            double v = 0;
            in >> f >> v;
            if (f == "adaptive") p.adaptive = (int)v;
            else if (f == "auto_emit") p.auto_emit = v != 0;
            else if (f == "auto_search") p.auto_search = v != 0;
            else if (f == "host_rate") p.host_rate = v;
            else if (f == "kernel_ms_per_req") p.kernel_ms_per_req = v;
            else if (f == "fixed_ms_per_req") p.fixed_ms_per_req = v;
            else if (f == "emit_share") p.emit_share = v;
            else if (f == "emit_share_opt") p.emit_share_opt = v;
            else if (f == "base_minfill") p.base_minfill = v;
            else if (f == "gpu_emit") k.gpu_emit = (int)v;
            else if (f == "gpu_search") k.gpu_search = (int)v;
            else if (f == "minfill_above") k.minfill_above = v;
            else { std::fprintf(stderr, "unknown field %s\n", f.c_str()); return 2; }
        } else if (cmd == "start") {
            unsigned long long call; int threads, on, en; double pm, km, rq;
            in >> call >> threads >> pm >> km >> rq >> on >> en;
            k = p.call_start(call, threads, pm, km, rq, on != 0, en != 0, k);
        } else if (cmd == "share") {
            long long n; int whole, wave;
            in >> n >> whole >> wave;
            nd = p.device_share(n, whole != 0, wave != 0);
        } else if (cmd == "chunk") {
            long long n, d, chunk; double hm, dm; int wave;
            in >> n >> d >> hm >> dm >> chunk >> wave;
            ruled = p.after_mixed_chunk(n, d, hm, dm, chunk, wave != 0).ruled;
        } else if (cmd == "end") {
            long long B; double ms;
            in >> B >> ms;
            p.call_end(B, ms);
        } else { std::fprintf(stderr, "unknown command %s\n", cmd.c_str()); return 2; }
        std::printf("gpu_emit=%d gpu_search=%d minfill_above=%.17g auto_emit=%d auto_search=%d seeded=%d streak=%d seen_plan_ms=%.17g seen_kernel_ms=%.17g "
                    "seen_requests=%.17g host_rate=%.17g kernel_ms_per_req=%.17g fixed_ms_per_req=%.17g emit_share=%.17g nd=%lld ruled=%d\n",
                    k.gpu_emit, k.gpu_search, k.minfill_above, (int)p.auto_emit, (int)p.auto_search, (int)p.adaptive_seeded, p.host_bound_streak, p.seen_plan_ms,
                    p.seen_kernel_ms, p.seen_requests, p.host_rate, p.kernel_ms_per_req, p.fixed_ms_per_req, p.emit_share, nd, ruled);
    }
    return 0;
}
