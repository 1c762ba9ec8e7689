// SURVEY.md 8(f) f2, image half: the dataset's RandomResizedCrop(448, bicubic) + RandomHorizontalFlip + Grayscale on the device
// (ECAMP/Pre-training/module/pretrain_datasets.py:47-52,113-115), bit for bit what the host transform produces.
//
// The reference runs torchvision 0.14.1's transforms on PIL images: F.resized_crop = img.crop(box).resize((448, 448), BICUBIC), i.e.
// Pillow's two-pass antialiased resample (Pillow 10.4.0 pinned in environment.yml:85; src/libImaging/Resample.c, unchanged in the
// 12.2.0 of this image).  Restated here from that published algorithm -- the filter support is widened by the scale factor, the
// normalised double-precision coefficients become 22-bit fixed point (precompute_coeffs / normalize_coeffs_8bpc), a horizontal pass
// writes a uint8 intermediate (ImagingResampleHorizontal_8bpc: 2^21 + sum(pixel * coef) >> 22, clipped), a vertical pass the same
// (ImagingResampleVertical_8bpc) -- and pinned by tests against Pillow itself (tests/test_augment*.py: equal bytes).
// MIMIC-CXR-JPG radiographs are grayscale: the reference's RGB crop has three equal channels, each resampled by the same integer
// arithmetic, and Grayscale's L = (19595 R + 38470 G + 7471 B + 2^15) >> 16 returns that common value -- so one uint8 plane is the
// whole item before ToTensor / Normalize (the `image_u8` schema the model's kernels already read).
// Colour sources (the fundus tasks of the classification transforms): Pillow resamples an RGB image band by band with these
// coefficients and this uint8 intermediate, and Grayscale follows the resize -- so a colour sample keeps three planes through both
// passes and the vertical pass folds them with the formula above: the host's byte again.
//
// Host -> device: per sample only the bytes of the drawn box (contiguous uint8) and a table row; the host draws the boxes and flips
// from the torch RNG in torchvision's order (ecamp_amd/module/pretrain_datasets.py, finetune_datasets.py).
// ONE pipeline of three launches -- coefficients (double precision, no contraction: the rounding of every operation is Pillow's),
// horizontal pass (rows x out uint8 intermediate in the caller's workspace), vertical pass (+ flip) -> dst uint8 [B, out, out] -- behind
// one host launch path (rs_run) and one workspace layout (rs_carve), with FOUR table forms, one entry point each:
//   ecamp_resample_crops_u8      stride 6, BICUBIC: {byte offset of the box in `src`, h, w, flip, first row in the intermediate, unused}
//   ecamp_resample_boxes_u8      stride 10, BILINEAR or BICUBIC: the same five + {full_w, shift_w, full_h, shift_h, 0}
//   ecamp_resample_boxes_rgb_u8  the stride-10 row whose last column is the plane count (3: planar R, G, B), three-plane passes
//   ecamp_resample_shard_u8      stride 12: that row + {pitch, plane_pitch} -- the box lies where it is in an image of a shard that
//                                stays in device memory (`src` is the whole shard); every row is checked against the shard's size
#include "common.h"

#define RS_PRECISION_BITS 22

struct RsTab { long off, h, w, flip, row0, pad; };   // pad: column 9 of a stride-10 row -- 3: three planes (ecamp_resample_boxes_rgb_u8 alone reads it)

__device__ __forceinline__ double rs_bicubic(double x) {
#pragma clang fp contract(off)
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// Pillow's BILINEAR filter (Resample.c bilinear_filter: the triangle 1 - |x|, support 1): the classification transforms
// (ECAMP/Fine-tuning/Classification/utils/data_utils.py:20-34 through torchvision's defaults)
__device__ __forceinline__ double rs_bilinear(double x) {
#pragma clang fp contract(off)
    if (x < 0.0) x = -x;
    if (x < 1.0) return 1.0 - x;
    return 0.0;
}

#define RS_BILINEAR 0
#define RS_BICUBIC 1
template <int F> struct RsFilter;
template <> struct RsFilter<RS_BILINEAR> {
    static constexpr double support = 1.0;
    static __device__ __forceinline__ double f(double x) { return rs_bilinear(x); }
};
template <> struct RsFilter<RS_BICUBIC> {
    static constexpr double support = 2.0;
    static __device__ __forceinline__ double f(double x) { return rs_bicubic(x); }
};

// one thread per (sample, axis, output index): bounds {first input index, tap count} and `kmax` fixed-point taps (zero past the count).
// `tab`: rows of `stride` int64.  stride 6 (ecamp_resample_crops_u8): the RsTab row, every axis resized from its size to `out`.  stride 10
// (ecamp_resample_boxes_u8): {off, h, w, flip, row0, full_w, shift_w, full_h, shift_h, 0} -- output index x of an axis is index
// u = x + shift of a resize of that axis from its size to `full`; u outside [0, full) has no tap (the passes then write (2^21) >> 22 = 0:
// CenterCrop's zero padding).  The RsTab share of such a row, and its last column (the plane count of the colour entry point: the taps
// depend on h, w and the geometry only), are copied to `tab_out` for the two passes.
// stride 12 (ecamp_resample_shard_u8): the stride-10 row + {pitch, plane_pitch}, a box inside an image of a resident shard of `shard_bytes`
// bytes.  A long-lived allocation is addressed by the table, so every row is checked here (rs_row_in_shard); a row that fails has no tap on
// either axis and h = 0 in `tab_out` -- the passes read nothing for it and write zeros, the padding path above -- and ORs 2 into `err`.
__device__ __forceinline__ bool rs_row_in_shard(const long* t, long shard_bytes) {
    const long off = t[0], h = t[1], w = t[2], pitch = t[10], plane_pitch = t[11];
    if (h <= 0 || w <= 0 || pitch < w || off < 0 || plane_pitch < 0 || off > shard_bytes) return false;
    // off + (c - 1) plane_pitch + (h - 1) pitch + w <= shard_bytes without a product that could overflow: what is left shrinks term by term
    long left = shard_bytes - off;
    if (w > left) return false;
    left -= w;
    if (h - 1 > left / pitch) return false;
    left -= (h - 1) * pitch;
    return t[9] != 3 || plane_pitch <= left / 2;
}

template <int F>
__global__ __launch_bounds__(256) void resample_coef_kernel(const long* __restrict__ tab, int stride, RsTab* __restrict__ tab_out, int2* __restrict__ bounds,
                                                            int* __restrict__ coef, long B, int out, int kmax, long shard_bytes,
                                                            int* __restrict__ err) {
#pragma clang fp contract(off)
    const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= B * 2 * out) return;
    const int xx = (int)(id % out), axis = (int)((id / out) & 1);
    const long b = id / (2 * out);
    const long* t = tab + b * stride;
    const int inSize = (int)(axis == 0 ? t[2] : t[1]);
    int full = out, u = xx;
    int* k = coef + id * kmax;
    if (stride >= 10) {
        full = (int)t[5 + 2 * axis];
        u = xx + (int)t[6 + 2 * axis];
        const bool ok = stride != 12 || rs_row_in_shard(t, shard_bytes);
        if (xx == 0 && axis == 0) {
            tab_out[b] = RsTab{t[0], ok ? t[1] : 0, t[2], t[3], t[4], t[9]};
            if (!ok) atomicOr(err, 2);
        }
        if (!ok) {   // a row that points outside the shard: no tap, as padding
            for (int x = 0; x < kmax; ++x) k[x] = 0;
            bounds[id] = make_int2(0, 0);
            return;
        }
    }
    if (full <= 0 || inSize <= 0) {
        if (xx == 0) atomicOr(err, 1);
        bounds[id] = make_int2(0, 0);
        return;
    }
    double scale = (double)inSize / (double)full, filterscale = scale;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = RsFilter<F>::support * filterscale;
    const int ksize = (int)ceil(support) * 2 + 1;
    if (ksize > kmax) {   // the host sized the tables for a smaller scale factor: refuse loudly (caller reads err)
        if (xx == 0) atomicOr(err, 1);
        bounds[id] = make_int2(0, 0);
        return;
    }
    if (u < 0 || u >= full) {   // padding: no tap
        for (int x = 0; x < kmax; ++x) k[x] = 0;
        bounds[id] = make_int2(0, 0);
        return;
    }
    const double center = 0 + (u + 0.5) * scale;
    const double ss = 1.0 / filterscale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > inSize) xmax = inSize;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) ww += RsFilter<F>::f((x + xmin - center + 0.5) * ss);
    for (int x = 0; x < kmax; ++x) {
        int q = 0;
        if (x < xmax) {
            double w = RsFilter<F>::f((x + xmin - center + 0.5) * ss);
            if (ww != 0.0) w /= ww;
            q = w < 0 ? (int)(-0.5 + w * (double)(1 << RS_PRECISION_BITS)) : (int)(0.5 + w * (double)(1 << RS_PRECISION_BITS));
        }
        k[x] = q;
    }
    bounds[id] = make_int2(xmin, xmax);
}

__device__ __forceinline__ unsigned char rs_clip8(int v) {
    v >>= RS_PRECISION_BITS;
    return (unsigned char)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// horizontal pass: block = (sample, chunk of ROWS rows); thread xx owns output column xx, its taps live in LDS as [tap][column].
// PLANES (the colour entry point): a sample of three planes h x w back to back is 3 h rows of w bytes, resampled row by row alike.
// PITCHED (ecamp_resample_shard_u8): the box lies inside a stored image -- row r of plane p starts at off + p * plane_pitch + r * pitch, the two
// pitches read from columns 10 and 11 of the caller's stride-12 row `ptab` (the coefficient kernel has checked the row against the shard's
// size, and a row that failed has no rows here).  The only pass that reads `src`: the intermediate is packed as before.
#define RS_ROWS 32
template <bool PLANES, bool PITCHED>
__global__ __launch_bounds__(512) void resample_h_kernel(const unsigned char* __restrict__ src, const RsTab* __restrict__ tab, const long* __restrict__ ptab,
                                                         const int2* __restrict__ bounds, const int* __restrict__ coef, unsigned char* __restrict__ tmp, int out,
                                                         int kmax) {
    extern __shared__ int kl[];   // [kmax][out]
    const long b = blockIdx.y;
    const RsTab t = tab[b];
    const int r0 = blockIdx.x * RS_ROWS;
    const int rows = PLANES && t.pad == 3 ? 3 * (int)t.h : (int)t.h;
    if (r0 >= rows) return;
    const long cid = (b * 2 + 0) * out;
    for (int i = threadIdx.x; i < out * kmax; i += blockDim.x) {
        const int xx = i / kmax, tp = i - xx * kmax;
        kl[tp * out + xx] = coef[(cid + xx) * kmax + tp];
    }
    __syncthreads();
    const int xx = threadIdx.x;
    if (xx >= out) return;
    const int2 bd = bounds[cid + xx];
    const int r1 = min(r0 + RS_ROWS, rows);
    const long pitch = PITCHED ? ptab[b * 12 + 10] : t.w, plane_pitch = PITCHED ? ptab[b * 12 + 11] : t.h * t.w;
    int pl = PITCHED ? r0 / (int)t.h : 0, pr = r0 - pl * (int)t.h;   // (plane, row in it) of intermediate row r; not PITCHED: r itself
    for (int r = r0; r < r1; ++r, ++pr) {
        if (PITCHED && pr == (int)t.h) { pr = 0; ++pl; }
        const unsigned char* p = src + t.off + (PITCHED ? pl * plane_pitch + pr * pitch : (long)r * t.w) + bd.x;
        int ss = 1 << (RS_PRECISION_BITS - 1);
        for (int tp = 0; tp < bd.y; ++tp) ss += (int)p[tp] * kl[tp * out + xx];
        tmp[(t.row0 + r) * out + xx] = rs_clip8(ss);
    }
}

// vertical pass (+ horizontal flip): block = (sample, output row); the row's taps are the same for every thread
__global__ __launch_bounds__(512) void resample_v_kernel(const unsigned char* __restrict__ tmp, const RsTab* __restrict__ tab, const int2* __restrict__ bounds,
                                                         const int* __restrict__ coef, unsigned char* __restrict__ dst, int out, int kmax) {
    const long b = blockIdx.y;
    const int yy = blockIdx.x, xx = threadIdx.x;
    if (xx >= out) return;
    const RsTab t = tab[b];
    const long cid = (b * 2 + 1) * out + yy;
    const int2 bd = bounds[cid];
    const int* k = coef + cid * kmax;
    const unsigned char* p = tmp + (t.row0 + bd.x) * out + xx;
    int ss = 1 << (RS_PRECISION_BITS - 1);
    for (int tp = 0; tp < bd.y; ++tp) ss += (int)p[(long)tp * out] * k[tp];
    dst[(b * out + yy) * out + (t.flip ? out - 1 - xx : xx)] = rs_clip8(ss);
}

// vertical pass of the colour entry point (+ luma fold + flip).  A three-plane sample owns 3 h rows of the intermediate, plane p from
// row0 + p h: the three clipped bytes of an output pixel come from the same taps, and Pillow's convert("L") folds them,
// L = (19595 R + 38470 G + 7471 B + 2^15) >> 16 (at most 65536 * 255 + 2^15: int32).  No tap: three zeros, and 2^15 >> 16 = 0.  A one-plane
// sample stores resample_v_kernel's byte.  One thread per output pixel, RS_VC_THREADS consecutive pixels of a sample per block: no lane
// is idle but in a sample's last block, at any `out` (a block per output row keeps 224 of 256 lanes at out = 224, 16 of 64 at out = 16).
#define RS_VC_THREADS 256
__global__ __launch_bounds__(RS_VC_THREADS) void resample_v_rgb_kernel(const unsigned char* __restrict__ tmp, const RsTab* __restrict__ tab,
                                                                       const int2* __restrict__ bounds, const int* __restrict__ coef,
                                                                       unsigned char* __restrict__ dst, int out, int kmax) {
    const long b = blockIdx.y;
    const int px = blockIdx.x * RS_VC_THREADS + threadIdx.x;
    if (px >= out * out) return;
    const int yy = px / out, xx = px - yy * out;
    const RsTab t = tab[b];
    const long cid = (b * 2 + 1) * out + yy;
    const int2 bd = bounds[cid];
    const int* k = coef + cid * kmax;
    const unsigned char* p = tmp + (t.row0 + bd.x) * out + xx;
    int v;
    if (t.pad == 3) {
        const long plane = t.h * out;
        int sr = 1 << (RS_PRECISION_BITS - 1), sg = sr, sb = sr;
        for (int tp = 0; tp < bd.y; ++tp) {
            const int kv = k[tp];
            const unsigned char* q = p + (long)tp * out;
            sr += (int)q[0] * kv;
            sg += (int)q[plane] * kv;
            sb += (int)q[2 * plane] * kv;
        }
        v = (19595 * (int)rs_clip8(sr) + 38470 * (int)rs_clip8(sg) + 7471 * (int)rs_clip8(sb) + 0x8000) >> 16;
    } else {
        int ss = 1 << (RS_PRECISION_BITS - 1);
        for (int tp = 0; tp < bd.y; ++tp) ss += (int)p[(long)tp * out] * k[tp];
        v = rs_clip8(ss);
    }
    dst[(b * out + yy) * out + (t.flip ? out - 1 - xx : xx)] = (unsigned char)v;
}

// ---- host side: one workspace layout and one launch path under the three entry points --------------------------------------------
static void rs_lds_optin() {
    static bool optin = false;
    if (!optin) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(resample_h_kernel<false, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(resample_h_kernel<true, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(resample_h_kernel<true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        optin = true;
    }
}

// workspace: bounds int2 [B][2][out] | coef int32 [B][2][out][kmax] | 256 spare bytes | intermediate uint8 [tmp_rows][out] | RsTab [B]
// (the stride-10 forms only); every part starts on a multiple of 256 bytes, `bytes` is the end of the last one
struct RsWorkspace { int2* bounds; int* coef; unsigned char* tmp; RsTab* tab; size_t bytes; };

static size_t rs_align(size_t v) { return (v + 255) & ~(size_t)255; }
static RsWorkspace rs_carve(void* ws, int64_t B, int out, int kmax, int64_t tmp_rows, bool with_tab) {
    const uintptr_t w = reinterpret_cast<uintptr_t>(ws);   // integers: the size functions carve a null workspace
    const size_t coef = rs_align((size_t)B * 2 * out * sizeof(int2)), tmp = coef + rs_align((size_t)B * 2 * out * kmax * sizeof(int)) + 256;
    const size_t tab = tmp + rs_align((size_t)tmp_rows * out), end = with_tab ? tab + rs_align((size_t)B * sizeof(RsTab)) : tab;
    return {reinterpret_cast<int2*>(w), reinterpret_cast<int*>(w + coef), reinterpret_cast<unsigned char*>(w + tmp),
            with_tab ? reinterpret_cast<RsTab*>(w + tab) : nullptr, end};
}

extern "C" int64_t ecamp_resample_crops_workspace_bytes(int64_t B, int32_t out, int32_t kmax, int64_t tmp_rows) {
    return B <= 0 || out <= 0 || kmax <= 0 || tmp_rows <= 0 ? 0 : (int64_t)rs_carve(nullptr, B, out, kmax, tmp_rows, false).bytes;
}

extern "C" int64_t ecamp_resample_boxes_workspace_bytes(int64_t B, int32_t out, int32_t kmax, int64_t tmp_rows) {
    return B <= 0 || out <= 0 || kmax <= 0 || tmp_rows <= 0 ? 0 : (int64_t)rs_carve(nullptr, B, out, kmax, tmp_rows, true).bytes;
}

// an entry point: its name (for messages), the stride of its table rows (6: the passes read the caller's table, no RsTab tail; 10: the
// coefficient kernel copies the RsTab share into the workspace tail; 12: the same, and the horizontal pass reads the two pitches from the
// caller's row), filter, smallest tap table, whether the passes are the three-plane ones, and the size of the resident shard (stride 12)
struct RsPlan { const char* name; int stride, filter, min_kmax; bool colour; int64_t shard_bytes; };

static int rs_run(const RsPlan& p, const uint8_t* src, const int64_t* table, uint8_t* dst, int64_t B, int32_t out, int32_t kmax, int64_t tmp_rows, int32_t max_h,
                  void* ws, int64_t ws_bytes, int32_t* err_flag, hipStream_t stream) {
    ECAMP_CHECK_ARG(src && table && dst && ws && err_flag, "%s: null argument", p.name);
    ECAMP_CHECK_ARG(p.filter == RS_BILINEAR || p.filter == RS_BICUBIC, "%s: filter %d (0: bilinear, 1: bicubic)", p.name, p.filter);
    const bool sizes_ok = B > 0 && B <= 65535 && out > 0 && out <= 512 && tmp_rows > 0 && max_h > 0 && max_h <= tmp_rows;   // B: gridDim.y of both passes
    ECAMP_CHECK_ARG(sizes_ok && kmax >= p.min_kmax && (size_t)kmax * out * sizeof(int) <= 160 * 1024,
                    "%s: B=%ld (<= 65535) out=%d (<= 512) kmax=%d (taps x out x 4 B must fit the 160 KB LDS) tmp_rows=%ld max_h=%d", p.name, (long)B, out, kmax, (long)tmp_rows, max_h);
    const bool with_tab = p.stride >= 10;
    const RsWorkspace k = rs_carve(ws, B, out, kmax, tmp_rows, with_tab);
    ECAMP_CHECK_ARG(ws_bytes >= (int64_t)k.bytes, "%s: workspace of %ld bytes is too small", p.name, (long)ws_bytes);
    const RsTab* tab = with_tab ? k.tab : reinterpret_cast<const RsTab*>(table);
    const long n = B * 2 * out;
    const auto coef_kernel = p.filter == RS_BILINEAR ? resample_coef_kernel<RS_BILINEAR> : resample_coef_kernel<RS_BICUBIC>;
    hipLaunchKernelGGL(coef_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, reinterpret_cast<const long*>(table), p.stride, k.tab, k.bounds, k.coef, (long)B,
                       (int)out, (int)kmax, (long)p.shard_bytes, (int*)err_flag);
    // rows per sample are data (the table lives on the device): the grid covers the tallest sample of the batch (max_h, the host knows it)
    const size_t shm = (size_t)kmax * out * sizeof(int);
    rs_lds_optin();
    const dim3 hgrid((unsigned)((max_h + RS_ROWS - 1) / RS_ROWS), (unsigned)B);
    const long* no_pitch = nullptr;
    if (p.colour) {
        if (p.stride == 12)
            hipLaunchKernelGGL((resample_h_kernel<true, true>), hgrid, dim3(512), shm, stream, src, tab, reinterpret_cast<const long*>(table), k.bounds, k.coef, k.tmp, (int)out,
                               (int)kmax);
        else
            hipLaunchKernelGGL((resample_h_kernel<true, false>), hgrid, dim3(512), shm, stream, src, tab, no_pitch, k.bounds, k.coef, k.tmp, (int)out, (int)kmax);
        const unsigned vblocks = (unsigned)(((long)out * out + RS_VC_THREADS - 1) / RS_VC_THREADS);
        hipLaunchKernelGGL(resample_v_rgb_kernel, dim3(vblocks, (unsigned)B), dim3(RS_VC_THREADS), 0, stream, k.tmp, tab, k.bounds, k.coef, dst, (int)out, (int)kmax);
    } else {
        hipLaunchKernelGGL((resample_h_kernel<false, false>), hgrid, dim3(512), shm, stream, src, tab, no_pitch, k.bounds, k.coef, k.tmp, (int)out, (int)kmax);
        hipLaunchKernelGGL(resample_v_kernel, dim3((unsigned)out, (unsigned)B), dim3(512), 0, stream, k.tmp, tab, k.bounds, k.coef, dst, (int)out, (int)kmax);
    }
    const hipError_t e = hipGetLastError();   // ECAMP_LAUNCH_CHECK with the entry point's name in place of __func__
    if (e != hipSuccess) return ecamp_set_error((int)e, "ecamp_%s: launch failed: %s", p.name, hipGetErrorString(e));
    return 0;
}

// the pre-training crops: stride-6 rows, BICUBIC, every axis resized from its size to `out`.  B <= 65535 (gridDim.y of the passes) is an
// argument error here as in the two entry points below: unchecked, a larger batch surfaces as a launch failure.
extern "C" int ecamp_resample_crops_u8(const uint8_t* src, const int64_t* table, uint8_t* dst, int64_t B, int32_t out, int32_t kmax, int64_t tmp_rows,
                                       int32_t max_h, void* ws, int64_t ws_bytes, int32_t* err_flag, hipStream_t stream) {
    return rs_run({"resample_crops_u8", 6, RS_BICUBIC, 5, false, 0}, src, table, dst, B, out, kmax, tmp_rows, max_h, ws, ws_bytes, err_flag, stream);
}

// the classification transforms (data_utils.py:20-34): RandomResizedCrop((s, s)) / flip, and Resize(int) + CenterCrop((s, s)).  One
// resample per axis with two more numbers: `full`, the size the axis is resized to, and `shift`, where the s output pixels start in
// that resized axis (negative, or past `full`: CenterCrop's zero padding).  Training is full = out, shift = 0 on the crop box.
extern "C" int ecamp_resample_boxes_u8(const uint8_t* src, const int64_t* table, uint8_t* dst, int64_t B, int32_t out, int32_t kmax, int64_t tmp_rows,
                                       int32_t max_h, int32_t filter, void* ws, int64_t ws_bytes, int32_t* err_flag, hipStream_t stream) {
    return rs_run({"resample_boxes_u8", 10, filter, filter == RS_BICUBIC ? 5 : 3, false, 0}, src, table, dst, B, out, kmax, tmp_rows, max_h, ws, ws_bytes, err_flag, stream);
}

// the same transforms on COLOUR sources: Grayscale (convert("L")) comes after the resize in data_utils.py:20-34, so the fold sits behind the
// vertical pass (resampling the gray plane instead differs by 1 in about 30 % of the bytes).  Column 9 of a table row is the plane count c: 3 = planar
// R, G, B (3 x h x w bytes at `off`, 3 h intermediate rows from row0), anything else the row of ecamp_resample_boxes_u8; tmp_rows / max_h count c * h.
extern "C" int ecamp_resample_boxes_rgb_u8(const uint8_t* src, const int64_t* table, uint8_t* dst, int64_t B, int32_t out, int32_t kmax, int64_t tmp_rows,
                                           int32_t max_h, int32_t filter, void* ws, int64_t ws_bytes, int32_t* err_flag, hipStream_t stream) {
    return rs_run({"resample_boxes_rgb_u8", 10, filter, filter == RS_BICUBIC ? 5 : 3, true, 0}, src, table, dst, B, out, kmax, tmp_rows, max_h, ws, ws_bytes, err_flag, stream);
}

// the same transforms on a shard that STAYS in device memory: `shard` is the whole uploaded file, a stride-12 row is the row above + {pitch,
// plane_pitch}, and `off` is where the box's first pixel lies in its stored image -- no box is copied, a loader worker sends the row alone.
// The three-plane passes serve both kinds of sample (column 9).  Only the horizontal pass reads `shard`; the coefficient kernel checks every
// row against `shard_bytes` first (rs_row_in_shard: a row that fails gives zeros and err_flag |= 2; 1 stays "more than kmax taps").
// With pitch = w, plane_pitch = h w and a packed source: the bytes of ecamp_resample_boxes_rgb_u8.
extern "C" int ecamp_resample_shard_u8(const uint8_t* shard, int64_t shard_bytes, const int64_t* table, uint8_t* dst, int64_t B, int32_t out, int32_t kmax,
                                       int64_t tmp_rows, int32_t max_h, int32_t filter, void* ws, int64_t ws_bytes, int32_t* err_flag, hipStream_t stream) {
    ECAMP_CHECK_ARG(shard_bytes > 0, "resample_shard_u8: shard_bytes=%ld (> 0)", (long)shard_bytes);
    return rs_run({"resample_shard_u8", 12, filter, filter == RS_BICUBIC ? 5 : 3, true, shard_bytes}, shard, table, dst, B, out, kmax, tmp_rows, max_h, ws, ws_bytes,
                  err_flag, stream);
}
