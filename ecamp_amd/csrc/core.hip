// Error reporting + ABI version for libecamp_hip.so
#include "common.h"
#include "attention.h"
#include "options.h"
#include "../../include/ecamp_hip.h"
#include <atomic>
#include <stdarg.h>
#include <stdlib.h>

thread_local char g_ecamp_err[512] = {0};

int ecamp_set_error(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_ecamp_err, sizeof(g_ecamp_err), fmt, ap);
    va_end(ap);
    return code;
}

extern "C" const char* ecamp_last_error(void) { return g_ecamp_err; }
extern "C" int ecamp_abi_version(void) { return ECAMP_ABI_VERSION; }
// 0: dtype code ECAMP_BF16 means bfloat16 (libecamp_hip.so); 1: it means IEEE half (libecamp_hip_f16.so, built with -DECAMP_HALF_F16)
extern "C" int ecamp_half_format(void) { return ECAMP_HALF_IS_F16; }

// ---- the switches (options.h).  `set`: what ecamp_set_option stores for a value (OPT_ENV: nothing, back to the environment); null: the
// switch has no option name.  INTEGRATION.md "Library options" is written from this table.
#define OPT_UNREAD (INT_MIN + 1)
struct OptRow {
    const char* name; const char* env; int def; int (*set)(int);
    std::atomic<int> value{OPT_ENV};          // the explicit value; OPT_ENV = none
    std::atomic<int> env_value{OPT_UNREAD};   // the environment's value or the default; OPT_UNREAD until first use
};
static OptRow g_opts[OPT_COUNT] = {
    // the eight-wave persistent kernel: -1 automatic, 0 never, 2 whenever legal.  Quirk, kept: a value other than 0 or 2 means AUTOMATIC,
    // not "the environment's value" -- once the option has been set, ECAMP_GEMM_Q8 is no longer consulted
    /* OPT_Q8_MODE */          {"q8_mode", "ECAMP_GEMM_Q8", -1, [](int v) { return v == 0 || v == 2 ? v : -1; }},
    // the four-wave kernel: 0 never, 1 where the 192-column tile pays, 2 every eligible call, 3 (tests) as 2 whatever the size
    /* OPT_Q16_MODE */         {"q16_mode", "ECAMP_Q16", 1, [](int v) { return v >= 0 && v <= 3 ? v : OPT_ENV; }},
    // the four-wave kernel's weight-gradient form (gemm_q16.h, q16w_body): 0 never, 1 the classes the measurements keep (gemm.hip,
    // q16_wgrad_on), 2 wherever legal (lab, tests); anything else: back to the environment
    /* OPT_Q16_WGRAD */        {"q16_wgrad", "ECAMP_Q16_WGRAD", 1, [](int v) { return v >= 0 && v <= 2 ? v : OPT_ENV; }},
    /* OPT_F8_Q8 */            {nullptr, "ECAMP_F8_Q8", 1, nullptr},             // 0: the 128^2 e4m3 kernel everywhere
    /* OPT_Q8_MIN_ITEMS */     {nullptr, "ECAMP_Q8_MIN_ITEMS", OPT_AUTO, nullptr},   // 256^2 work items from which Q8 is chosen; default half the CU count
    // workgroups of the data-gradient form (gemm.hip, gemm_select); 0 = one per CU, and back to the environment
    /* OPT_Q8_BWD_GRID */      {"q8_bwd_grid", "ECAMP_Q8_BWD_GRID", 0, [](int v) { return v > 0 ? v : OPT_ENV; }},
    /* OPT_P8_WGRAD */         {"p8_wgrad", nullptr, 1, [](int v) { return v ? 1 : 0; }},   // 0: weight gradients stay off the persistent kernel
    /* OPT_P8_WGRAD_RESERVE */ {"p8_wgrad_reserve_cus", nullptr, 0, [](int v) { return v < 0 ? 0 : v; }},   // CUs the backward-pass forms leave free
    /* OPT_WGRAD_ITEMS */      {nullptr, "ECAMP_WGRAD_ITEMS", 0, nullptr},       // work items a weight-gradient split is chosen for; 0 = CU count
    /* OPT_WGRAD_GROUP_CUS */  {nullptr, "ECAMP_WGRAD_GROUP_CUS", 0, nullptr},   // workgroups of the grouped launch; 0 = 3/4 of the CUs, capped by the reserve
    /* OPT_GEMM_GRID_CAP */    {nullptr, "ECAMP_GEMM_GRID_CAP", 0, nullptr},     // development: CU count the persistent GEMMs assume (>= 32, below the real one)
    // 1 head-resident attention kernels, 0 the 64-row streaming kernels for every length; negative: back to the environment
    /* OPT_ATTN_HEAD */        {"attn_head", "ECAMP_ATTN_HEAD", 1, [](int v) { return v < 0 ? OPT_ENV : v ? 1 : 0; }},
    /* OPT_ATTN_WAVES */       {nullptr, "ECAMP_ATTN_WAVES", 0, nullptr},        // > 0: cap of the waves per head-kernel workgroup (tuning)
    /* OPT_LN_BWD */           {nullptr, "ECAMP_LN_BWD", 0, nullptr},            // development: 1 = the 4-wide LayerNorm backward forms only
    /* OPT_SR_BLOCKS */        {nullptr, "ECAMP_SR_BLOCKS", 512, nullptr},       // development: grid of the paired super-resolution backward (two workgroups per CU)
};
int ecamp_opt_default(EcampOpt id) { return g_opts[id].def; }
int ecamp_opt(EcampOpt id) {
    OptRow& o = g_opts[id];
    const int s = o.value.load(std::memory_order_relaxed);
    if (s != OPT_ENV) return s;
    int e = o.env_value.load(std::memory_order_relaxed);
    if (e == OPT_UNREAD) {
        const char* txt = o.env ? getenv(o.env) : nullptr;
        e = txt ? atoi(txt) : o.def;
        o.env_value.store(e, std::memory_order_relaxed);
    }
    return e;
}
bool ecamp_opt_set(const char* name, int value) {
    for (OptRow& o : g_opts)
        if (o.name && strcmp(name, o.name) == 0) {
            o.value.store(o.set(value), std::memory_order_relaxed);
            return true;
        }
    return false;
}
extern "C" int ecamp_set_option(const char* name, int32_t value) {
    ECAMP_CHECK_ARG(name != nullptr, "set_option: null name");
    if (strcmp(name, "attn_head") == 0) { attn_set_head_mode(value); return 0; }   // the attention module's own entry (attention_bf16.hip)
    if (ecamp_opt_set(name, value)) return 0;
    return ecamp_set_error(-1, "set_option: unknown option '%s'", name);
}

// Development aid (tools/hog_probe.py): `blocks` workgroups that spin for `cycles` shader clocks -- a stand-in for a communication
// kernel (RCCL all-reduce) that shares the GPU with the training step on another stream.
__global__ void dev_spin_kernel(long long cycles) {
    const long long t0 = clock64();
    while (clock64() - t0 < cycles) {}
}
extern "C" int ecamp_dev_spin(int32_t blocks, int32_t threads, int64_t cycles, hipStream_t stream) {
    ECAMP_CHECK_ARG(blocks > 0 && threads > 0 && threads <= 1024 && cycles >= 0, "dev_spin: bad arguments");
    hipLaunchKernelGGL(dev_spin_kernel, dim3(blocks), dim3(threads), 0, stream, (long long)cycles);
    ECAMP_LAUNCH_CHECK();
    return 0;
}
