// `prog_sim draw` under its former name and command line: g++ -O2 -mpopcnt -std=c++17 -ffp-contract=off tools/draw_sim.cpp sorobn_amd/csrc/planner.cpp -lpthread
#define PROG_SIM_KIND "draw"
#include "prog_sim.cpp"
