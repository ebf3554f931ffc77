// Reference-shaped caller of the fall test through the C++ shim: what main.cpp:48-50 arms
// (set_flag("torso_kicks", true), set_fall_test(hc, tmin, tmax)) around position control, then
// simulate_ode until fall_check (player.cpp:669-681) would print its line and exit. The shim
// reports the verdict through fall_state() instead of exiting.
//   fall_test <models> <dvx> <dvy> <dvz> <kick_every> <kick_phase> <hc> <tmin> <tmax> <steps> [torque_limit]
#include <cstdio>
#include <cstdlib>
#include <string>

#include "hslabs.hpp"

using namespace hslabs;

int main(int argc, char** argv) {
  if (argc < 11) return 2;
  std::string models = argv[1];
  const double dv[3] = {std::atof(argv[2]), std::atof(argv[3]), std::atof(argv[4])};
  const int every = std::atoi(argv[5]), phase = std::atoi(argv[6]);
  const double hc = std::atof(argv[7]), tmin = std::atof(argv[8]), tmax = std::atof(argv[9]);
  const int steps = std::atoi(argv[10]);
  modelplayer player;
  pergensetup* pgs = player.make_pergensu(models + "/pgs_config.txt", 8, models);
  bool threw = false;
  try {
    player.set_flag("no_such_flag", true);
  } catch (const error&) {
    threw = true;
  }
  std::printf("unknown_flag_throws = %d\n", threw ? 1 : 0);
  player.set_flag("torso_kicks", true);
  player.set_torso_kick(dv, every, phase);
  player.set_fall_test(hc, tmin, tmax);
  if (argc > 11) player.set_torque_limit(std::atof(argv[11]));
  player.setup_per_controller(pgs, 0.02);
  // the visualizer's loop (player.cpp:55-62) in chunks of 25 steps: a frozen world takes no more steps
  for (int done = 0; done < steps; done += 25) player.simulate_ode(steps - done < 25 ? steps - done : 25);
  modelplayer::fall_result r = player.fall_state();
  if (r.fallen) std::printf("Fall at t = %.6f\n", r.t);
  else if (r.survived) std::printf("No fall by t = %.6f\n", r.t);
  else std::printf("Running at t = %.6f\n", r.t);
  double p[3];
  player.get_torso_pos(p);
  std::printf("play_t = %.6f\n", player.get_play_t());
  std::printf("torso = %.12f %.12f %.12f\n", p[0], p[1], p[2]);
  std::printf("below_hc = %d\n", player.fall_check(hc) ? 1 : 0);
  delete pgs;
  return 0;
}
