// `prog_sim map` under its former name and command line: g++ -O2 -mpopcnt -std=c++17 -ffp-contract=off tools/map_sim.cpp sorobn_amd/csrc/planner.cpp -lpthread
#define PROG_SIM_KIND "map"
#include "prog_sim.cpp"
