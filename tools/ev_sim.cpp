// `prog_sim ev` under its former name and command line: g++ -O2 -mpopcnt -std=c++17 -ffp-contract=off tools/ev_sim.cpp sorobn_amd/csrc/planner.cpp -lpthread
#define PROG_SIM_KIND "ev"
#include "prog_sim.cpp"
