// hs_oracle_f32.cpp -- TEST INFRASTRUCTURE ONLY: the oracle (hs_oracle.cpp with hs_oracle_sim.cpp)
// compiled with every `double` an f32r (f32round.h): the restatement's own answer in single
// precision, the reference the fp32 simulation kernels are bounded by
// (tests/test_sim_oracle_f32.py, tests/test_gpu_sim_f32_oracle.py). Same exports, same double*
// arrays as libhs_oracle.so; oracle.py's lib_f32() binds it and Model(path, L=lib_f32()) owns a
// model of it.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <map>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "f32round.h"

// HSO_FLOPCOUNT leaves the near-rank diagnostics out (they are not arithmetic of the path) and
// with them the simulation include, which therefore follows by name
#define HSO_FLOPCOUNT 1
// solve_forces' rank guard is the kernel's float kFastPivotGuard (1e-4), not the fp64 1e-10
#define HSO_F32_BUILD 1
#define double f32r
#include "hs_oracle.cpp"
#include "hs_oracle_sim.cpp"
#undef double
