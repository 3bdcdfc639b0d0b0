// TEST INFRASTRUCTURE ONLY — the three Config members that include2/config.h declares and its inline
// getters need, defined here so that src2/config.cpp (yaml, boost) stays out of the build. Every field a
// pinned function reads is set through the reference's own getters by refpin_shim.cpp before each call.
#include "config.h"

Config::Config() : best_lr_matches(true), matching_s_ws(0), matching_f2f_ws(0), min_ratio_12_p(0.0), line_sim_th(0.0) {}
Config::~Config() {}
Config &Config::getInstance() { static Config instance; return instance; }
