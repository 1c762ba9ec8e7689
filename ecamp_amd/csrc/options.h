// Process-wide switches of libecamp_hip.so: ONE table (core.hip, g_opts) with, for each switch, its ecamp_set_option name, its
// environment variable, its default and the rule ecamp_set_option applies to a value.  Kernel code reads a switch by enum index.
#pragma once
#include <limits.h>

enum EcampOpt {
    OPT_Q8_MODE, OPT_Q16_MODE, OPT_Q16_WGRAD, OPT_F8_Q8, OPT_Q8_MIN_ITEMS, OPT_Q8_BWD_GRID, OPT_P8_WGRAD, OPT_P8_WGRAD_RESERVE,
    OPT_WGRAD_ITEMS, OPT_WGRAD_GROUP_CUS, OPT_GEMM_GRID_CAP, OPT_ATTN_HEAD, OPT_ATTN_WAVES, OPT_LN_BWD, OPT_SR_BLOCKS, OPT_COUNT
};
#define OPT_ENV INT_MIN    // result of a value rule: forget the explicit value, the environment (or the default) decides again
#define OPT_AUTO INT_MIN   // default of a switch whose default depends on the device (the reader derives it)

#define ECAMP_HIDDEN __attribute__((visibility("hidden")))
// the value in force: the last ecamp_set_option value if its rule kept one, else the environment variable (read once, at first use,
// with atoi), else the default
ECAMP_HIDDEN int ecamp_opt(EcampOpt id);
ECAMP_HIDDEN int ecamp_opt_default(EcampOpt id);
// ecamp_set_option's lookup by name: false if no switch has that option name
ECAMP_HIDDEN bool ecamp_opt_set(const char* name, int value);
