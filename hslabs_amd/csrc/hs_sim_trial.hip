// hs_sim_trial.hip -- the fall test's instantiations of the simulation kernel (hs_sim_trial: open-loop
// torques, torque limit, torso kicks, fall check) and the tally of its state array, compiled apart
// from hs_sim_step's so that those stay the code they were (see hs_sim.hip).
#define HS_SIM_TRIAL_TU 1
#include "hs_sim.hip"
