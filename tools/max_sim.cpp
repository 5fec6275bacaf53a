// `prog_sim max` under its former name and command line: g++ -O2 -mpopcnt -std=c++17 -ffp-contract=off tools/max_sim.cpp sorobn_amd/csrc/planner.cpp -lpthread
#define PROG_SIM_KIND "max"
#include "prog_sim.cpp"
