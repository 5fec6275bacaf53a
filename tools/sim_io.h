// What tools/dag_plan_sim.cpp and tools/dag_post_sim.cpp share: reading white-space separated input from stdin, the candidate
// list both take, and printing lists into their JSON output.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

inline long long geti() {
    long long v;
    if (!(std::cin >> v)) { std::fprintf(stderr, "input ends early\n"); std::exit(2); }
    return v;
}
inline double getd() {  // by strtod: nan, inf, 0x1p-3 ..
    std::string tok;
    if (!(std::cin >> tok)) { std::fprintf(stderr, "input ends early\n"); std::exit(2); }
    return std::strtod(tok.c_str(), nullptr);
}
inline unsigned long long bits_of(double x) {
    unsigned long long u;
    std::memcpy(&u, &x, 8);
    return u;
}
// , "key": [item(a[0]), item(a[1]), ..] as unsigned integers
template <class T, class F>
void put_list(const char *key, const std::vector<T> &a, F &&item) {
    std::printf(", \"%s\": [", key);
    for (size_t i = 0; i < a.size(); ++i) std::printf(i ? ", %llu" : "%llu", (unsigned long long)item(a[i]));
    std::printf("]");
}
inline void put_bits(const char *key, const std::vector<double> &a) { put_list(key, a, bits_of); }

// the head of both inputs: n_vars tile_bits group_bits tables n_fam, then n_fam triples  child parent_mask score
struct SimInput {
    int32_t n;
    int tile_bits, group_bits;
    bool tables;
    int64_t n_fam;
    std::vector<int32_t> child;
    std::vector<uint32_t> parents;
    std::vector<double> score;
};
inline SimInput read_sim_input() {
    SimInput in;
    in.n = (int32_t)geti();
    in.tile_bits = (int)geti();
    in.group_bits = (int)geti();
    in.tables = geti() != 0;
    in.n_fam = geti();
    if (in.n_fam < 0) { std::fprintf(stderr, "n_fam is negative\n"); std::exit(2); }
    for (int64_t f = 0; f < in.n_fam; ++f) {
        in.child.push_back((int32_t)geti());
        in.parents.push_back((uint32_t)geti());
        in.score.push_back(getd());
    }
    return in;
}
