// Shared argument block of the attention kernels (attention.hip: exact-f32 MFMA path; attention_bf16.hip: bf16 MFMA path).
#pragma once
#include "common.h"

struct AttnArgs {
    const void* q; const void* k; const void* v; void* o;
    const void* dout; void* dq; void* dk; void* dv;
    float* lse; float* delta;
    const int32_t* key_mask;  // [B, Tk], nonzero = attend; or null
    long q_sb, q_st, q_sh, k_sb, k_st, k_sh, v_sb, v_st, v_sh, o_sb, o_st, o_sh;
    long dq_sb, dq_st, dq_sh, dk_sb, dk_st, dk_sh, dv_sb, dv_st, dv_sh, do_sb, do_st, do_sh;
    int B, H, Tq, Tk;
    float scale, drop_p;
    uint64_t seed, offset;
    // Dropout keep-mask of the attention probabilities as BITS, written by the head-resident forward kernel and read by its backward
    // (one Philox evaluation per score instead of three); null: every kernel regenerates the mask from the Philox counters.
    // Layout [B*H][Tq][4][8] bytes: byte (row, g, pp) = keys pp*32 + 4g + r (bits r = 0..3) and pp*32 + 16 + 4g + r (bits 4 + r).
    unsigned char* drop_bits;
};

#define NEG_BIG (-1.0e30f)

#define LDS_MAX (160 * 1024)   // the LDS of one CU: the most a workgroup can be given

// 64-key chunks of a key range whose scores a kernel instantiation keeps in accumulator registers (template parameter KCH); 0: more than 256 keys
static inline int attn_kch(int Tk) { return Tk <= 64 ? 1 : Tk <= 128 ? 2 : Tk <= 256 ? 4 : 0; }

// Dynamic LDS of the head-resident 16-bit kernels (attention_bf16.hip, attn_head_*_kernel), the one statement of it: two images of `prow` rows of
// hd 16-bit elements (forward: K, V; backward: K, V and then Q, dO over the same area, so the longer of the two sequences counts), rows in
// whole pairs of 16-row tiles; per row the f32 key bias, in the backward pass also lse and delta, and with saved dropout bits 32 bytes.
static inline size_t head_lds_bytes(int Tq, int Tk, int hd, bool backward, bool bits) {
    const int nkp = ((Tk + 15) / 16 + 1) / 2, nqp = ((Tq + 15) / 16 + 1) / 2;
    const size_t prow = (size_t)(backward && nqp > nkp ? nqp : nkp) * 32;
    return 2 * prow * (2 * hd) + (backward ? 3 : 1) * prow * sizeof(float) + (backward && bits ? 32 * prow : 0);
}

// What attn_select answers and attn_launch runs: one launch, or two for a backward pass outside the head-resident family (dQ, then dK / dV).
enum AttnFamily { ATTN_HEAD, ATTN_RESIDENT_FWD, ATTN_STREAM, ATTN_LONG, ATTN_F32 };
typedef void (*AttnKernel)(AttnArgs);
struct AttnLaunch {
    AttnFamily family;
    int n, block;   // launches; threads per workgroup
    // what the profiler tag says beside the call's shape (attn_tag, attention.hip): the KCH the kernel is instantiated on (-1: it has none),
    // FLAGS (key mask or dropout), and whether saved dropout bits are written (forward) or read (backward) -- head-resident kernels only
    int kch, flags, bits;
    // lds: dynamic LDS of this call.  optin: the size the kernel is allowed once, at its first launch, if it is more than 48 KB (0: never) --
    // for the head kernels the largest size any later call may ask for, not this call's.
    struct Kernel { AttnKernel fn; dim3 grid; size_t lds, optin; } k[2];
};
#define ATTN_HD_SWITCH(hd, F, ...) ((hd) == 32 ? F<32>(__VA_ARGS__) : (hd) == 64 ? F<64>(__VA_ARGS__) : F<128>(__VA_ARGS__))

// attention_bf16.hip: the 16-bit half of attn_select (it stands next to its kernels), and the one launcher of both files
ECAMP_HIDDEN AttnLaunch attn16_select(int B, int H, int Tq, int Tk, int hd, bool mask_or_dropout, bool bits, bool backward);
ECAMP_HIDDEN void attn_launch(const AttnLaunch& l, const AttnArgs& a, hipStream_t st);
void attn_set_head_mode(int on);   // ecamp_set_option("attn_head", ...): -1 back to the environment's choice
