"""Thin tensor-level wrappers over the C ABI (include/ecamp_hip.h).  torch is used ONLY for device memory
(`torch.empty`) and the current HIP stream handle; every FLOP / byte moved below happens in libecamp_hip.so.
No CPU fallback exists: CPU tensors raise."""
import ctypes
import os

import torch

from . import _lib, streams
from ._lib import BF16, F32, call

_I64x3 = ctypes.c_int64 * 3


def code(dtype):
    if dtype == torch.float32:
        return F32
    if dtype == torch.bfloat16 or dtype == torch.float16:
        want = "bf16" if dtype == torch.bfloat16 else "f16"
        if _lib.half() != want:   # the 16-bit format is a property of the loaded build, not of the call: the wrong one would reinterpret the bits
            raise TypeError("a %s tensor reached the %s build of libecamp_hip -- call ecamp_amd._lib.set_half(%r) first "
                            "(ECAMP(compute_dtype=...) does)" % (dtype, _lib.half(), want))
        return BF16
    raise TypeError("ecamp_amd supports float32, bfloat16 and float16 activations, got %s" % dtype)


def _chk(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.EcampHipError("ecamp_amd ops need tensors on an MI355X (HIP) device; got a CPU tensor. "
                                     "There is no CPU fallback in the product path.")


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


# --------------------------------------------------------------------------------------------- gemm
def gemm(A, B, C, M, N, K, a_kc, lda, b_kc, ldb, ldc, bias=None, residual=None, ldr=0, pre_out=None, ldp=0, gmul=None,
         ldg=0, act=0, alpha=1.0, alpha_dev=None, out_f32=False, accumulate=False, split_k=1, rowsum=None):
    _chk(A, B, C)
    nws = int(_lib.load().ecamp_gemm_workspace_bytes(M, N, K, int(split_k))) // 4
    ws = torch.empty((nws,), device=A.device, dtype=torch.float32) if nws > 0 else None
    call("ecamp_gemm", ptr(A), ptr(B), ptr(C), M, N, K, int(a_kc), lda, int(b_kc), ldb, ldc, ptr(bias), ptr(residual), ldr,
         ptr(pre_out), ldp, ptr(gmul), ldg, int(act), float(alpha), ptr(alpha_dev), code(A.dtype), int(out_f32), int(accumulate), int(split_k),
         ptr(ws), ptr(rowsum), stream())
    return C


def linear_fwd(x, w, bias=None, act=0, residual=None, save_pre=False, out_dtype=None):
    """y = act(x @ w.T + bias) (+ residual);  x [M,K] (K-contiguous rows), w [N,K] in x.dtype."""
    M, K = x.shape
    N = w.shape[0]
    assert w.shape[1] == K and x.stride(1) == 1 and w.stride(1) == 1 and w.dtype == x.dtype
    out_f32 = out_dtype == torch.float32 and x.dtype != torch.float32
    y = torch.empty((M, N), device=x.device, dtype=torch.float32 if out_f32 else x.dtype)
    pre = torch.empty((M, N), device=x.device, dtype=x.dtype) if save_pre else None
    gemm(x, w, y, M, N, K, True, x.stride(0), True, w.stride(0), N, bias=bias, residual=residual,
         ldr=residual.stride(0) if residual is not None else 0, pre_out=pre, ldp=N, act=act, out_f32=out_f32)
    return (y, pre) if save_pre else y


def linear_fwd_res32(x, w, bias, residual):
    """y (f32) = x @ w.T + bias + residual (f32) -- the residual linear layers of the f32 residual stream (ECAMP(f32_residual=True)):
    16-bit operands, the sum formed in f32 and never rounded to 16 bits.  x [M,K], w [N,K] 16-bit; residual [M,N] f32."""
    _chk(x, w, residual)
    M, K = x.shape
    N = w.shape[0]
    assert w.shape[1] == K and x.stride(1) == 1 and w.stride(1) == 1 and w.dtype == x.dtype and x.dtype != torch.float32
    assert residual.dtype == torch.float32 and residual.shape == (M, N) and residual.stride(1) == 1
    y = torch.empty((M, N), device=x.device, dtype=torch.float32)
    call("ecamp_gemm_res32", ptr(x), ptr(w), ptr(y), M, N, K, x.stride(0), w.stride(0), N, ptr(bias), ptr(residual), residual.stride(0),
         code(x.dtype), stream())
    return y


# --------------------------------------------------------------------------------------------- fp8 forward (configs[4])
def quantize_fp8(x):
    """Per-tensor e4m3 quantisation of a contiguous f32/bf16 tensor (numel % 4 == 0): -> (q uint8 same shape, scale f32[1]);
    x ~= q * scale, scale = max|x| / 448 taken from THIS tensor (current scaling: two passes, no history)."""
    _chk(x)
    assert x.is_contiguous()
    amax = torch.empty((1,), device=x.device, dtype=torch.float32)
    zero_(amax)
    call("ecamp_amax", ptr(x), ptr(amax), x.numel(), code(x.dtype), stream())
    q = torch.empty(x.shape, device=x.device, dtype=torch.uint8)
    scale = torch.empty((1,), device=x.device, dtype=torch.float32)
    call("ecamp_quant_fp8", ptr(x), ptr(amax), ptr(q), ptr(scale), x.numel(), code(x.dtype), stream())
    return q, scale


def fp8_roll(amax_slots, scale, hist=None, hist_pos=0, margin=1.0):
    """Once per optimizer step: scale[i] = margin * max(site i's 16 amax slots, its history) / 448 where a producer fed the site; slots = 0.
    hist: optional f32 [sites, k] ring of the last k maxima (delayed scaling of activation sites); None + margin 1 = exact current scaling."""
    call("ecamp_fp8_roll", ptr(amax_slots), ptr(scale), scale.numel(), ptr(hist), hist.shape[1] if hist is not None else 0, int(hist_pos),
         float(margin), stream())


def fp8_weights(w16, w8, items, amax_slots, scales, pass_):
    """One pass of the whole-arena weight quantisation (ParamArena._quantize_weights): 0 = per-matrix maxima, 1 = quantise."""
    call("ecamp_fp8_weights", ptr(w16), ptr(w8), ptr(items), items.shape[0], ptr(amax_slots), ptr(scales), int(pass_), stream())


def quantize_fp8_site(x, scale, amax_slots, calibrated):
    """e4m3 copy of x for a GEMM-input site (ParamArena.f8_site).  Calibrated: ONE pass -- quantise with the site's scale (the
    previous step's maximum), record this step's maximum.  First use: the two-pass current scaling, which seeds scale and slots."""
    assert x.is_contiguous() and x.numel() % 4 == 0
    q = torch.empty(x.shape, device=x.device, dtype=torch.uint8)
    if calibrated:
        call("ecamp_quant_fp8_delayed", ptr(x), ptr(scale), ptr(q), ptr(amax_slots), x.numel(), code(x.dtype), stream())
    else:
        call("ecamp_amax", ptr(x), ptr(amax_slots), x.numel(), code(x.dtype), stream())
        call("ecamp_quant_fp8", ptr(x), ptr(amax_slots), ptr(q), ptr(scale), x.numel(), code(x.dtype), stream())
    return q


def gemm_fp8(x8, x_scale, w8, w_scale, bias=None, act=0, residual=None, save_pre=False, q8_site=None):
    """y (bf16) = act(dequant(x8) @ dequant(w8).T + bias) (+ residual) on the e4m3 GEMM (ecamp_gemm_fp8): x8 [M,K], w8 [N,K] uint8.
    q8_site = (scale, amax slots) of the NEXT dense layer (GELU epilogue only): a third result, the e4m3 copy of y made in the epilogue."""
    M, K = x8.shape
    N = w8.shape[0]
    assert w8.shape[1] == K and w8.dtype == torch.uint8 and x8.dtype == torch.uint8 and x8.is_contiguous() and w8.is_contiguous()
    y = torch.empty((M, N), device=x8.device, dtype=torch.bfloat16)
    pre = torch.empty((M, N), device=x8.device, dtype=torch.bfloat16) if save_pre else None
    y8 = torch.empty((M, N), device=x8.device, dtype=torch.uint8) if q8_site is not None else None
    call("ecamp_gemm_fp8", ptr(x8), ptr(w8), ptr(y), M, N, K, K, K, N, ptr(x_scale), ptr(w_scale), ptr(bias), ptr(residual),
         residual.stride(0) if residual is not None else 0, ptr(pre), N, int(act), ptr(y8), ptr(q8_site[0] if q8_site else None),
         ptr(q8_site[1] if q8_site else None), stream())
    if q8_site is not None:
        return y, pre, y8
    return (y, pre) if save_pre else y


def linear_fwd_fp8(x, w8, w_scale, bias=None, act=0, residual=None, save_pre=False):
    """y (bf16) = act(dequant(q(x)) @ dequant(w8).T + bias) (+ residual): x [M,K] bf16 is quantised here, w8 [N,K] uint8 + scale
    come from `quantize_fp8(weight)` (once per optimizer step).  The backward of the layer keeps using the bf16 x and w."""
    M, K = x.shape
    N = w8.shape[0]
    assert w8.shape[1] == K and w8.dtype == torch.uint8 and x.dtype == torch.bfloat16 and x.is_contiguous() and w8.is_contiguous()
    x8, xs = quantize_fp8(x)
    y = torch.empty((M, N), device=x.device, dtype=torch.bfloat16)
    pre = torch.empty((M, N), device=x.device, dtype=torch.bfloat16) if save_pre else None
    call("ecamp_gemm_fp8", ptr(x8), ptr(w8), ptr(y), M, N, K, K, K, N, ptr(xs), ptr(w_scale), ptr(bias), ptr(residual),
         residual.stride(0) if residual is not None else 0, ptr(pre), N, int(act), ptr(None), ptr(None), ptr(None), stream())
    return (y, pre) if save_pre else y


def linear_dgrad(dy, w, gmul=None, alpha=1.0, alpha_dev=None, residual=None, gmul_is_grad=False):
    """dx = alpha * (dy @ w) [* gelu'(gmul)] [+ residual];  dy [M,N], w [N,K].  gmul_is_grad: `gmul` is what a forward with act=2 saved,
    gelu' itself (ecamp_gemm act = 2), and multiplies the result as it is."""
    M, N = dy.shape
    K = w.shape[1]
    dx = torch.empty((M, K), device=dy.device, dtype=dy.dtype)
    gemm(dy, w, dx, M, K, N, True, dy.stride(0), False, w.stride(0), K, gmul=gmul, ldg=gmul.stride(0) if gmul is not None else 0,
         residual=residual, ldr=residual.stride(0) if residual is not None else 0, alpha=alpha, alpha_dev=alpha_dev,
         act=2 if (gmul_is_grad and gmul is not None) else 0)
    return dx


_SPLIT_CACHE = {}
_WG_TABLES = {}   # (device, shapes, has_bias, rows, workgroups) -> device image of a weight-gradient group's item table (uploaded once, kept)


def set_option(name, value):
    """ecamp_set_option + invalidation of the split-count cache (the suggested split depends on the kernel selection)."""
    call("ecamp_set_option", name.encode(), int(value))
    _SPLIT_CACHE.clear()
    _WG_TABLES.clear()     # the grouped weight gradients' item tables depend on the CU reserve


def _split_k(n_out, k_in, m, dtype=torch.bfloat16):
    """Split count of the weight-gradient GEMM (M=n_out, N=k_in, K=m): asked of the library, which knows which kernel runs."""
    key = (n_out, k_in, m, dtype)
    s = _SPLIT_CACHE.get(key)
    if s is None:
        s = _SPLIT_CACHE[key] = max(1, int(_lib.load().ecamp_gemm_suggest_split(n_out, k_in, m, 0, 0, code(dtype))))
    return s


def linear_wgrad(dy, x, gw, alpha=1.0, alpha_dev=None, gb=None, accumulate=True):
    """gw[N,K] (f32) += (accumulate) or = alpha * dy[M,N]^T @ x[M,K];  gb[N] (f32, always accumulated) += alpha * sum_m dy[m,:] if given."""
    M, N = dy.shape
    K = x.shape[1]
    assert gw.dtype == torch.float32 and gw.is_contiguous() and gw.numel() == N * K
    gemm(dy, x, gw, N, K, M, False, dy.stride(0), False, x.stride(0), K, alpha=alpha, alpha_dev=alpha_dev, out_f32=True,
         accumulate=bool(accumulate), split_k=_split_k(N, K, M, dy.dtype), rowsum=gb)


WGRAD_GROUP = os.environ.get("ECAMP_WGRAD_GROUP", "1") != "0"   # one launch per transformer block for its weight gradients


def wgrad_group_supported(items):
    """items: [(dy, x, gw, gb or None, accumulate)] -- can they run as one grouped launch (same row count, bf16, aligned shapes)?"""
    if not WGRAD_GROUP or not 1 <= len(items) <= 4:
        return False
    rows = items[0][0].shape[0]
    for dy, x, gw, gb, _ in items:
        if dy.dtype not in (torch.bfloat16, torch.float16) or x.dtype != dy.dtype or dy.shape[0] != rows or x.shape[0] != rows:
            return False
        if not (dy.is_contiguous() and x.is_contiguous() and gw.is_contiguous() and gw.dtype == torch.float32):
            return False
    n = len(items)
    no = (ctypes.c_int64 * n)(*[it[0].shape[1] for it in items])
    ki = (ctypes.c_int64 * n)(*[it[1].shape[1] for it in items])
    return bool(_lib.load().ecamp_wgrad_group_supported(n, ctypes.cast(no, ctypes.c_void_p), ctypes.cast(ki, ctypes.c_void_p), rows))


def _wgrad_group_table(dev, n, no, ki, hb, rows, workgroups):
    lib = _lib.load()
    nwg = int(lib.ecamp_wgrad_group_workgroups(int(workgroups)))
    key = (str(dev), tuple(no), tuple(ki), tuple(hb), int(rows), nwg)
    t = _WG_TABLES.get(key)
    if t is None:
        cv = lambda a: ctypes.cast(a, ctypes.c_void_p)
        cap = int(lib.ecamp_wgrad_group_table_bytes(n, cv(no), cv(ki), rows))
        host = torch.empty((cap,), dtype=torch.uint8)
        used = int(lib.ecamp_wgrad_group_table(n, cv(no), cv(ki), cv((ctypes.c_int32 * n)(*hb)), rows, int(workgroups), ctypes.c_void_p(host.data_ptr())))
        if used <= 0:
            raise _lib.EcampHipError("ecamp_wgrad_group_table failed: %s" % lib.ecamp_last_error().decode())
        # one-time upload on the current stream (a blocking copy from pageable memory: the first call for a shape set, never in a captured region)
        t = _WG_TABLES[key] = host[:used].to(dev)
    return t


def wgrad_group(items, alpha=1.0, alpha_dev=None, workgroups=0):
    """gw_p [N_p, K_p] (f32) (+)= alpha * dy_p^T x_p and gb_p += alpha * column sums of dy_p for every (dy, x, gw, gb, accumulate) of
    `items` in ONE persistent launch + one reduce (ecamp_wgrad_group): the weight gradients of one transformer block."""
    n = len(items)
    rows = items[0][0].shape[0]
    no = (ctypes.c_int64 * n)(*[it[0].shape[1] for it in items])
    ki = (ctypes.c_int64 * n)(*[it[1].shape[1] for it in items])
    vp = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() if t is not None else None for t in ts])
    dyp, xp, gwp, gbp = vp([it[0] for it in items]), vp([it[1] for it in items]), vp([it[2] for it in items]), vp([it[3] for it in items])
    acc = (ctypes.c_int32 * n)(*[1 if it[4] else 0 for it in items])
    cv = lambda a: ctypes.cast(a, ctypes.c_void_p)
    dev = items[0][0].device
    table = _wgrad_group_table(dev, n, no, ki, [1 if it[3] is not None else 0 for it in items], rows, workgroups)
    nws = int(_lib.load().ecamp_wgrad_group_workspace_bytes(n, cv(no), cv(ki), rows)) // 4
    ws = torch.empty((nws,), device=dev, dtype=torch.float32)
    call("ecamp_wgrad_group", n, cv(dyp), cv(xp), cv(gwp), cv(gbp), cv(no), cv(ki), rows, float(alpha), ptr(alpha_dev), cv(acc), ptr(ws), ptr(table),
         table.numel(), int(workgroups), stream())


def colsum(x, out, alpha=1.0, period=0, lo=0, hi=0, alpha_dev=None):
    """out[N] (f32) += alpha * sum_m x[m, :]  (optionally only rows with lo <= m % period < hi)."""
    _chk(x, out)
    M, N = x.shape
    call("ecamp_colsum", ptr(x), x.stride(0), M, N, float(alpha), ptr(alpha_dev), period, lo, hi, ptr(out), code(x.dtype), stream())


# --------------------------------------------------------------------------------------------- layernorm
def layernorm_fwd(x, gamma, beta, eps, residual=None, drop_p=0.0, seed=0, offset=0, q8_site=None):
    """-> (y, z, mean, rstd);  z is x itself unless residual/dropout are fused (then the materialised LN input).
    q8_site = (scale f32[1], amax slots f32[512]) of the GEMM that consumes y (fp8 forward, calibrated site): a fifth result, the e4m3
    copy of y quantised inside this kernel (ecamp_layernorm_fwd_q8)."""
    _chk(x, gamma, beta)
    rows, cols = x.shape
    assert x.is_contiguous()
    y = torch.empty_like(x)
    mean = torch.empty(rows, device=x.device, dtype=torch.float32)
    rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
    fused = residual is not None or drop_p > 0.0
    z = torch.empty_like(x) if fused else None
    if q8_site is not None:
        y8 = torch.empty((rows, cols), device=x.device, dtype=torch.uint8)
        call("ecamp_layernorm_fwd_q8", ptr(x), ptr(residual), ptr(z), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd), rows, cols,
             float(eps), float(drop_p), seed, offset, ptr(y8), ptr(q8_site[0]), ptr(q8_site[1]), code(x.dtype), stream())
        return y, (z if fused else x), mean, rstd, y8
    call("ecamp_layernorm_fwd", ptr(x), ptr(residual), ptr(z), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd), rows, cols,
         float(eps), float(drop_p), seed, offset, code(x.dtype), stream())
    return y, (z if fused else x), mean, rstd


def layernorm_bwd(dy, z, mean, rstd, gamma, ggamma, gbeta, dres=None, drop_p=0.0, seed=0, offset=0, want_drop=False):
    """-> dz (+dres) [, dz through the dropout mask];  ggamma/gbeta (f32) are accumulated."""
    rows, cols = dy.shape
    assert dy.is_contiguous() and z.is_contiguous()
    dz = torch.empty_like(dy)
    dxd = torch.empty_like(dy) if want_drop else None
    call("ecamp_layernorm_bwd", ptr(dy), ptr(z), ptr(mean), ptr(rstd), ptr(gamma), ptr(dres), ptr(dz), ptr(dxd), ptr(ggamma),
         ptr(gbeta), rows, cols, float(drop_p), seed, offset, code(dy.dtype), stream())
    return (dz, dxd) if want_drop else dz


def layernorm_fwd_x32(x, gamma, beta, eps, dtype):
    """LayerNorm of an f32 row (the f32 residual stream) with a 16-bit output `dtype`: -> (y, x, mean, rstd) like layernorm_fwd."""
    _chk(x, gamma, beta)
    rows, cols = x.shape
    assert x.is_contiguous() and x.dtype == torch.float32
    y = torch.empty((rows, cols), device=x.device, dtype=dtype)
    mean = torch.empty(rows, device=x.device, dtype=torch.float32)
    rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
    call("ecamp_layernorm_fwd_x32", ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd), rows, cols, float(eps), code(dtype), stream())
    return y, x, mean, rstd


def layernorm_bwd_z32(dy, z, mean, rstd, gamma, ggamma, gbeta, dres=None):
    """layernorm_bwd of a LayerNorm whose input z is f32 (layernorm_fwd_x32); dy, dres and the result dz are 16-bit."""
    rows, cols = dy.shape
    assert dy.is_contiguous() and z.is_contiguous() and z.dtype == torch.float32 and (dres is None or dres.dtype == dy.dtype)
    dz = torch.empty_like(dy)
    call("ecamp_layernorm_bwd_z32", ptr(dy), ptr(z), ptr(mean), ptr(rstd), ptr(gamma), ptr(dres), ptr(dz), ptr(ggamma), ptr(gbeta), rows, cols,
         code(dy.dtype), stream())
    return dz


def layernorm_layout(backward, rows16, cols, al16=True, opt_bwd=0):
    """-> (vec, chunks, waves, greg, lds, grid_cap): the layout the library selects for such a call (ecamp_layernorm_layout; host
    arithmetic, nothing is launched).  rows16: 16-bit rows, the f32-stream entries included; al16: every row pointer 16-byte aligned."""
    out = (ctypes.c_int32 * 6)()
    call("ecamp_layernorm_layout", int(bool(backward)), int(bool(rows16)), int(cols), int(bool(al16)), int(opt_bwd),
         ctypes.cast(out, ctypes.c_void_p))
    return (out[0], out[1], out[2], bool(out[3]), out[4], out[5])


# --------------------------------------------------------------------------------------------- attention
def _st(t3):
    return _I64x3(*t3)


def attn_fwd(q, k, v, B, H, Tq, Tk, hd, qs, ks, vs, scale, key_mask=None, drop_p=0.0, seed=0, offset=0, want_mask=False):
    """q/k/v: tensors whose storage is addressed with element strides (batch, token, head); returns (o [B,Tq,H*hd], lse) and, with
    `want_mask`, the dropout keep-mask as bits (uint8 tensor, or None where the bit form does not apply) for `attn_bwd`."""
    _chk(q, k, v)
    o = torch.empty((B, Tq, H * hd), device=q.device, dtype=q.dtype)
    lse = torch.empty((B, H, Tq), device=q.device, dtype=torch.float32)
    bits = None
    if want_mask and drop_p > 0.0:
        nb = int(_lib.load().ecamp_attn_mask_bytes(B, H, Tq, Tk, hd, code(q.dtype)))
        if nb > 0:
            bits = torch.empty((nb,), device=q.device, dtype=torch.uint8)
    call("ecamp_attn_fwd", ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), ptr(key_mask), B, H, Tq, Tk, hd, _st(qs), _st(ks), _st(vs),
         _st((Tq * H * hd, H * hd, hd)), float(scale), float(drop_p), seed, offset, code(q.dtype), ptr(bits), stream())
    return (o, lse, bits) if want_mask else (o, lse)


def attn_probs(q, k, B, H, Tq, Tk, hd, qs, ks, scale, key_mask=None):
    """softmax(scale * q k^T [+ finfo.min on masked keys]) -> f32 [B, H, Tq, Tk]  (Visualization/module/context_fusion.py:45-57)."""
    _chk(q, k)
    probs = torch.empty((B, H, Tq, Tk), device=q.device, dtype=torch.float32)
    call("ecamp_attn_probs", ptr(q), ptr(k), ptr(key_mask), ptr(probs), B, H, Tq, Tk, hd, _st(qs), _st(ks), float(scale), code(q.dtype), stream())
    return probs


def attn_bwd(q, k, v, o, do, lse, dq, dk, dv, B, H, Tq, Tk, hd, qs, ks, vs, dqs, dks, dvs, scale, key_mask=None, drop_p=0.0,
             seed=0, offset=0, drop_bits=None):
    delta = torch.empty((B, H, Tq), device=q.device, dtype=torch.float32)
    os_ = (Tq * H * hd, H * hd, hd)
    assert do.is_contiguous() and o.is_contiguous()
    call("ecamp_attn_bwd", ptr(q), ptr(k), ptr(v), ptr(o), ptr(do), ptr(lse), ptr(delta), ptr(dq), ptr(dk), ptr(dv), ptr(key_mask),
         B, H, Tq, Tk, hd, _st(qs), _st(ks), _st(vs), _st(os_), _st(os_), _st(dqs), _st(dks), _st(dvs), float(scale), float(drop_p),
         seed, offset, code(q.dtype), ptr(drop_bits), stream())


# --------------------------------------------------------------------------------------------- misc
def add(a, b):
    _chk(a, b)
    y = torch.empty_like(a)
    call("ecamp_add", ptr(a), ptr(b), ptr(y), a.numel(), code(a.dtype), stream())
    return y


def mul_gelu_grad(dy, pre):
    _chk(dy, pre)
    dx = torch.empty_like(dy)
    call("ecamp_gelu_bwd", ptr(dy), ptr(pre), ptr(dx), dy.numel(), code(dy.dtype), stream())
    return dx


def cast(src, dst):
    _chk(src, dst)
    call("ecamp_cast", ptr(src), ptr(dst), src.numel(), code(src.dtype), code(dst.dtype), stream())
    return dst


def scale_(x, alpha=1.0, alpha_dev=None):
    """x *= alpha * alpha_dev[0] in place (f32 arithmetic, any activation dtype)."""
    _chk(x, alpha_dev)
    assert x.is_contiguous() and x.numel() % 4 == 0
    call("ecamp_scale", ptr(x), ptr(x), x.numel(), float(alpha), ptr(alpha_dev), code(x.dtype), stream())
    return x


def zero_blocks_(g, flags):
    """Zero the 64-element blocks of the f32 arena `g` whose byte in `flags` (uint8, len = g.numel() / 64) is non-zero."""
    _chk(g, flags)
    call("ecamp_zero_blocks", ptr(g), ptr(flags), g.numel(), stream())


def zero_(t):
    _chk(t)
    call("ecamp_zero", ptr(t), t.numel() * t.element_size(), stream())
    return t


def zeros(shape, device, dtype=torch.float32):
    return zero_(torch.empty(shape, device=device, dtype=dtype))


def bcast_add(x, g):
    B, S, H = x.shape
    y = torch.empty_like(x)
    call("ecamp_bcast_add", ptr(x), ptr(g), ptr(y), B, S, H, code(x.dtype), stream())
    return y


def seq_sum(x, s0, s1, scale):
    B, S, H = x.shape
    out = torch.empty((B, H), device=x.device, dtype=x.dtype)
    call("ecamp_seq_sum", ptr(x), ptr(out), B, S, H, s0, s1, float(scale), code(x.dtype), stream())
    return out


def seq_bcast(g, y, s0, s1, scale, mode):
    B, S, H = y.shape
    call("ecamp_seq_bcast", ptr(g), ptr(y), B, S, H, s0, s1, float(scale), mode, code(y.dtype), stream())
    return y


def dropout_mask(shape, device, p, seed, offset):
    """Development ABI: the keep-mask (uint8, 1 = kept) of a tensor of `shape` under dropout(p) keyed by (seed, offset) -- what the
    LayerNorm / embedding / attention kernels regenerate from the same pair (element index = flat index of the contiguous tensor)."""
    out = torch.empty(shape, device=device, dtype=torch.uint8)
    call("ecamp_dropout_mask", ptr(out), out.numel(), float(p), seed, offset, stream())
    return out


def drop_path_fwd(res, y, B, T, p, seed, offset, out=None):
    """Stochastic depth (timm DropPath, scale_by_keep): out[b] = res[b] + s_b * y[b] over [B*T, D] rows, s_b = 0 or 1 / (1 - p); sample b is
    kept iff dropout_mask((B,), dev, p, seed, offset)[b].  res and y 16-bit, both f32, or res f32 with a 16-bit y; `out` (res's dtype) is
    allocated unless given, and may be `y` itself when the dtypes agree."""
    _chk(res, y, out)
    M, D = res.shape
    assert M == B * T and y.shape == res.shape and res.is_contiguous() and y.is_contiguous()
    if out is None:
        out = torch.empty_like(res)
    assert out.shape == res.shape and out.dtype == res.dtype and out.is_contiguous()
    call("ecamp_drop_path_fwd", ptr(res), ptr(y), ptr(out), B, T, D, float(p), seed, offset, code(res.dtype), code(y.dtype), stream())
    return out


def drop_path_bwd(dout, B, T, p, seed, offset):
    """Gradient of drop_path_fwd with respect to y: s_b * dout[b] (a new tensor; the gradient of res is dout itself)."""
    _chk(dout)
    M, D = dout.shape
    assert M == B * T and dout.is_contiguous()
    dy = torch.empty_like(dout)
    call("ecamp_drop_path_bwd", ptr(dout), ptr(dy), B, T, D, float(p), seed, offset, code(dout.dtype), stream())
    return dy


def uniform(shape, device, seed, offset):
    out = torch.empty(shape, device=device, dtype=torch.float32)
    call("ecamp_uniform", ptr(out), out.numel(), seed, offset, stream())
    return out


# --------------------------------------------------------------------------------------------- image side
IMG_MEAN, IMG_STD = 0.4721, 0.3037   # the reference's Normalize (pretrain_datasets.py:52): one value for the three identical channels


_IMG_LUT = {}


def image_lut(device, mean=IMG_MEAN, std=IMG_STD):
    """lut[u] = ((float)u / 255 - mean) / std: ToTensor + Normalize of every byte value in their own f32 arithmetic (256 floats, built once
    per device and pair of constants; the default pair is pre-training's, the classifier passes finetune_datasets.FT_MEAN / FT_STD)."""
    key = (str(device), float(mean), float(std))
    t = _IMG_LUT.get(key)
    if t is None:
        t = _IMG_LUT[key] = torch.arange(256, dtype=torch.float32).div(255.0).sub(float(mean)).div(float(std)).to(device)
    return t


def is_u8_image(t):
    """The compact image schema: uint8 [B, H, W] (or [B, 1, H, W]) grayscale crops instead of normalised f32 [B, 3, H, W]."""
    return t.dtype == torch.uint8


def bicubic_resize(src, Hd, Wd):
    """f32 [B,C,Hs,Ws] -> f32 [B,C,Hd,Wd]; a uint8 [B,Hs,Ws] / [B,1,Hs,Ws] crop -> the normalised, resized f32 [B,3,Hd,Wd]."""
    _chk(src)
    if is_u8_image(src):
        src = src.reshape(src.shape[0], src.shape[-2], src.shape[-1])
        assert src.is_contiguous()
        B, Hs, Ws = src.shape
        dst = torch.empty((B, 3, Hd, Wd), device=src.device, dtype=torch.float32)
        call("ecamp_bicubic_resize_u8", ptr(src), ptr(dst), B, Hs, Ws, Hd, Wd, ptr(image_lut(src.device)), stream())
        return dst
    B, C, Hs, Ws = src.shape
    assert src.dtype == torch.float32 and src.is_contiguous()
    dst = torch.empty((B, C, Hd, Wd), device=src.device, dtype=torch.float32)
    call("ecamp_bicubic_resize", ptr(src), ptr(dst), B * C, Hs, Ws, Hd, Wd, stream())
    return dst


def mask_indices(noise, len_keep):
    _chk(noise)
    B, L = noise.shape
    ids_restore = torch.empty((B, L), device=noise.device, dtype=torch.int32)
    ids_keep = torch.empty((B, len_keep), device=noise.device, dtype=torch.int32)
    mask = torch.empty((B, L), device=noise.device, dtype=torch.float32)
    call("ecamp_mask_indices", ptr(noise), B, L, len_keep, ptr(ids_restore), ptr(ids_keep), ptr(mask), stream())
    return ids_restore, ids_keep, mask


def im2col_gather(imgs, ids_keep, p, dtype):
    B, C, R, _ = imgs.shape
    Lk = ids_keep.shape[1]
    out = torch.empty((B * (Lk + 1), C * p * p), device=imgs.device, dtype=dtype)
    call("ecamp_im2col_gather", ptr(imgs), ptr(ids_keep), ptr(out), B, Lk, C, R, p, code(dtype), stream())
    return out


def im2col_u8(img, lut, ids_keep, p, dtype):
    """im2col_gather straight from a uint8 grayscale image [B, R, R] at the model's own size, normalised through `lut` (image_lut): the bits
    of im2col_gather on lut[img] expanded to three planes, without that f32 image."""
    _chk(img, lut, ids_keep)
    assert img.dtype == torch.uint8 and img.dim() == 3 and img.shape[1] == img.shape[2] and img.is_contiguous()
    assert lut.dtype == torch.float32 and lut.numel() == 256 and lut.is_contiguous()
    B, R, _ = img.shape
    Lk = ids_keep.shape[1]
    out = torch.empty((B * (Lk + 1), 3 * p * p), device=img.device, dtype=dtype)
    call("ecamp_im2col_u8", ptr(img), ptr(lut), ptr(ids_keep), ptr(out), B, Lk, R, p, code(dtype), stream())
    return out


def assemble_tokens_(x, cls, pos, ids_keep, B, Lk, D):
    call("ecamp_assemble_tokens", ptr(x), ptr(cls), ptr(pos), ptr(ids_keep), B, Lk, D, code(x.dtype), stream())
    return x


def assemble_tokens_x32(x, cls, pos, ids_keep, B, Lk, D):
    """assemble_tokens_ into a NEW f32 tensor: the 16-bit patch-embed output x + the f32 position table (autocast's order)."""
    out = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    call("ecamp_assemble_tokens_x32", ptr(x), ptr(out), ptr(cls), ptr(pos), ptr(ids_keep), B, Lk, D, code(x.dtype), stream())
    return out


def unshuffle_fwd_x32(y, ids_restore, mask_token, dpos, B, L, Lk, D):
    """unshuffle_fwd with an f32 result: the 16-bit decoder_embed output or the f32 mask token, + the f32 position table."""
    xd = torch.empty((B, L + 1, D), device=y.device, dtype=torch.float32)
    call("ecamp_unshuffle_fwd_x32", ptr(y), ptr(ids_restore), ptr(mask_token), ptr(dpos), ptr(xd), B, L, Lk, D, code(y.dtype), stream())
    return xd


def unshuffle_fwd(y, ids_restore, mask_token, dpos, B, L, Lk, D):
    xd = torch.empty((B, L + 1, D), device=y.device, dtype=y.dtype)
    call("ecamp_unshuffle_fwd", ptr(y), ptr(ids_restore), ptr(mask_token), ptr(dpos), ptr(xd), B, L, Lk, D, code(y.dtype), stream())
    return xd


def unshuffle_bwd(dxd, ids_restore, ids_keep, gmask_token, B, L, Lk, D):
    dy = torch.empty((B, Lk + 1, D), device=dxd.device, dtype=dxd.dtype)
    call("ecamp_unshuffle_bwd", ptr(dxd), ptr(ids_restore), ptr(ids_keep), ptr(dy), ptr(gmask_token), B, L, Lk, D, code(dxd.dtype),
         stream())
    return dy


def unpatchify_mim(pred, imgs, mask, loss_sum, B, R, p):
    pred_img = torch.empty((B, 3, R, R), device=pred.device, dtype=torch.float32)
    call("ecamp_unpatchify_mim", ptr(pred), ptr(imgs), ptr(mask), ptr(pred_img), ptr(loss_sum), B, R, p, code(pred.dtype), stream())
    return pred_img


def img_loss_bwd(pred_img, imgs, mask, dsr, gm_gs, B, R, p, dtype):
    L = (R // p) ** 2
    dpred = torch.empty((B * (L + 1), p * p * 3), device=pred_img.device, dtype=dtype)
    call("ecamp_img_loss_bwd", ptr(pred_img), ptr(imgs), ptr(mask), ptr(dsr), ptr(gm_gs), ptr(dpred), B, R, p, code(dtype), stream())
    return dpred


def sr_fwd(pred_img, big, column, row, w1, b1, w2, b2, loss_sum, super_patch, window, mode=0):
    """mode 0: f32 stencils (parity); 1: bf16 matrix cores."""
    B, _, R, _ = pred_img.shape
    call("ecamp_sr_fwd", ptr(pred_img), ptr(big), ptr(image_lut(big.device) if is_u8_image(big) else None), ptr(column), ptr(row), ptr(w1), ptr(b1), ptr(w2), ptr(b2),
         ptr(loss_sum), B, R, super_patch, window, int(mode), stream())


def sr_image(pred_img, w1, b1, w2, b2):
    """super_res(pred_img): f32 [B,3,2R,2R] (parity / visualisation; the training step never materialises it)."""
    B, _, R, _ = pred_img.shape
    out = torch.empty((B, 3, 2 * R, 2 * R), device=pred_img.device, dtype=torch.float32)
    call("ecamp_sr_image", ptr(pred_img), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(out), B, R, stream())
    return out


def sr_bwd(pred_img, big, column, row, w1, b1, w2, b2, gw_ws, super_patch, window, mode=0):
    B, _, R, _ = pred_img.shape
    dsr = torch.empty((B, 3, R, R), device=pred_img.device, dtype=torch.float32)
    call("ecamp_sr_bwd", ptr(pred_img), ptr(big), ptr(image_lut(big.device) if is_u8_image(big) else None), ptr(column), ptr(row), ptr(w1), ptr(b1), ptr(w2), ptr(b2),
         ptr(dsr), ptr(gw_ws), B, R, super_patch, window, int(mode), stream())
    return dsr


def scaled_accum(ws, grad, scale_dev, idx):
    call("ecamp_scaled_accum", ptr(ws), ptr(grad), ptr(scale_dev), idx, ws.numel(), stream())


# --------------------------------------------------------------------------------------------- report side
def bert_embed_fwd(ids, type_ids, word, pos, typ, gamma, beta, eps, dtype, drop_p=0.0, seed=0, offset=0):
    _chk(ids, word)
    B, S = ids.shape
    H = word.shape[1]
    z = torch.empty((B * S, H), device=ids.device, dtype=dtype)
    e = torch.empty((B * S, H), device=ids.device, dtype=dtype)
    mean = torch.empty(B * S, device=ids.device, dtype=torch.float32)
    rstd = torch.empty(B * S, device=ids.device, dtype=torch.float32)
    call("ecamp_bert_embed_fwd", ptr(ids), ptr(type_ids), ptr(word), ptr(pos), ptr(typ), ptr(gamma), ptr(beta), ptr(z), ptr(e),
         ptr(mean), ptr(rstd), B, S, H, float(eps), float(drop_p), seed, offset, code(dtype), stream())
    return e, z, mean, rstd


def bert_embed_bwd(de, z, mean, rstd, gamma, ids, type_ids, gword, gpos, gtype, ggamma, gbeta, B, S, H, drop_p=0.0, seed=0,
                   offset=0, pad_id=0, hot=(2, 3)):
    call("ecamp_bert_embed_bwd", ptr(de), ptr(z), ptr(mean), ptr(rstd), ptr(gamma), ptr(ids), ptr(type_ids), ptr(gword), ptr(gpos),
         ptr(gtype), ptr(ggamma), ptr(gbeta), B, S, H, pad_id, hot[0], hot[1], float(drop_p), seed, offset, code(de.dtype), stream())


def ce_fwd_bwd_(logits, labels, weights, loss_sum, gain=1.0):
    """In place: logits -> gain * d(mean weighted CE)/d logits (unit upstream gradient); loss_sum += sum_i w_i CE_i.
    `gain` (a power of two the caller divides out of the upstream gradient again): the gradient is written in the logits' own format before
    the loss scale is known, and w (p - onehot) / M is 1e-9 for M = 32768 rows -- zero in IEEE half."""
    _chk(logits, labels, weights)
    M, V = logits.shape
    assert logits.stride(1) == 1 and labels.numel() == M and weights.numel() == M
    if M == 0:      # no rows (an empty tensor has no address to hand over)
        return logits
    call("ecamp_ce_fwd_bwd", ptr(logits), ptr(labels), ptr(weights), ptr(loss_sum), M, V, logits.stride(0), float(gain) / M,
         code(logits.dtype), stream())
    return logits


def ce_eval(logits, labels, weights):
    """Evaluation form of the head's loss (read-only on `logits` [M, V]): -> (loss_sum f32[1] = sum_i w_i CE_i over the rows whose label
    lies in [0, V), counts int64[3] = [rows scored, label ranks first, label within the first five]); rank = logits strictly above the
    label's.  Rows with an ignored label are never read."""
    _chk(logits, labels, weights)
    M, V = logits.shape
    assert logits.stride(1) == 1 and labels.numel() == M and weights.numel() == M
    loss_sum, counts = zeros((1,), logits.device), zeros((3,), logits.device, torch.int64)
    call("ecamp_ce_eval", ptr(logits), ptr(labels), ptr(weights), ptr(loss_sum), ptr(counts), M, V, logits.stride(0), code(logits.dtype), stream())
    return loss_sum, counts


COMPACT_GRANULE = 256   # rows: the capacity of a compacted head is a multiple of it (whole GEMM tiles; equal-sized batches reuse allocator blocks)


def compact_cap(count):
    """Capacity for `count` scored rows: rounded up to COMPACT_GRANULE, one granule of padding when nothing is scored."""
    return max(1, -(-int(count) // COMPACT_GRANULE)) * COMPACT_GRANULE


def compact_rows(x, labels, weights, ids=None, mask_id=3, vocab=None, cap=None):
    """The scored rows of x [M, cols] in front (ecamp_compact_rows): row m is scored iff 0 <= labels[m] < vocab and (ids is None or
    ids[m] == mask_id; 3 = [MASK], ecamp_amd.data.MASK) -> (x_c [cap, cols], labels_c int64[cap], weights_c f32[cap], rows int32[cap],
    count int64[1]): the scored rows in their order, `rows` their indices in x; rows [count, cap) are padding (zeros, -100, 0, -1).
    `count` is the true number of scored rows, on the device, also where it exceeds `cap` (then the first `cap` were written).
    cap=None: M, which always suffices."""
    _chk(x, labels, weights, ids)
    M, cols = x.shape
    assert vocab is not None and x.stride(1) == 1 and labels.numel() == M and weights.numel() == M and (ids is None or ids.numel() == M)
    assert labels.dtype == torch.int64 and weights.dtype == torch.float32 and (ids is None or ids.dtype == torch.int64)
    assert labels.is_contiguous() and weights.is_contiguous() and (ids is None or ids.is_contiguous())
    cap = M if cap is None else int(cap)
    dev = x.device
    x_c = torch.empty((cap, cols), device=dev, dtype=x.dtype)
    labels_c = torch.empty((cap,), device=dev, dtype=torch.int64)
    weights_c = torch.empty((cap,), device=dev, dtype=torch.float32)
    rows = torch.empty((cap,), device=dev, dtype=torch.int32)
    count = torch.empty((1,), device=dev, dtype=torch.int64)
    ws = torch.empty((int(_lib.load().ecamp_compact_rows_workspace_bytes(M)),), device=dev, dtype=torch.uint8)
    call("ecamp_compact_rows", ptr(x), x.stride(0), ptr(labels), ptr(weights), ptr(ids), int(mask_id), M, cols, int(vocab), cap, ptr(x_c),
         ptr(labels_c), ptr(weights_c), ptr(rows), ptr(count), ptr(ws), code(x.dtype), stream())
    return x_c, labels_c, weights_c, rows, count


# --------------------------------------------------------------------------------------------- linear probe (csrc/classify.hip)
def pool_norm(x, t0, t1, gamma=None, beta=None, eps=1e-6):
    """x [B, T, D] (16-bit or f32) -> (pooled, feat), both f32 [B, D]: the mean over tokens t0 <= t < t1 and its LayerNorm (gamma / beta
    f32, both None = identity affine), in one pass with f32 means (ecamp_pool_norm)."""
    _chk(x, gamma, beta)
    B, T, D = x.shape
    assert x.is_contiguous() and (gamma is None) == (beta is None)
    assert gamma is None or (gamma.dtype == torch.float32 and beta.dtype == torch.float32 and gamma.numel() == D and beta.numel() == D)
    pooled = torch.empty((B, D), device=x.device, dtype=torch.float32)
    feat = torch.empty((B, D), device=x.device, dtype=torch.float32)
    dt = code(x.dtype)
    ws = torch.empty((max(16, int(_lib.load().ecamp_pool_norm_workspace_bytes(B, T, D, int(t0), int(t1), dt))),), device=x.device, dtype=torch.uint8)
    call("ecamp_pool_norm", ptr(x), ptr(gamma), ptr(beta), ptr(pooled), ptr(feat), B, T, D, int(t0), int(t1), float(eps), ptr(ws), dt, stream())
    return pooled, feat


def cls_head_fwd(feat, w, bias):
    """logits f32 [B, C] = feat [B, D] . w [C, D]^T + bias [C], all f32, C <= 64."""
    _chk(feat, w, bias)
    B, D = feat.shape
    C = w.shape[0]
    assert feat.dtype == w.dtype == bias.dtype == torch.float32 and feat.is_contiguous() and w.is_contiguous() and bias.is_contiguous()
    assert w.shape == (C, D) and bias.numel() == C
    logits = torch.empty((B, C), device=feat.device, dtype=torch.float32)
    call("ecamp_cls_head_fwd", ptr(feat), ptr(w), ptr(bias), ptr(logits), B, C, D, stream())
    return logits


def cls_loss(logits, targets, kind, check=False):
    """kind 0: BCE with logits against f32 targets [B, C] (mean over B*C); kind 1: cross entropy against int64 labels [B] (mean over B)
    -> (loss f32[1], dlogits f32 [B, C] = gradient of that mean, counts int64[2] = [rows seen, rows predicted right], bad int32[1] = 1 if
    a kind-1 label lies outside [0, C)).  `bad` stays on the device for the caller to read where it synchronises anyway
    (`cls_check_labels`); check=True reads it here -- a synchronisation -- and raises."""
    _chk(logits, targets)
    B, C = logits.shape
    assert logits.dtype == torch.float32 and logits.is_contiguous() and targets.is_contiguous()
    if kind == 0:
        assert targets.dtype == torch.float32 and tuple(targets.shape) == (B, C), "kind 0: f32 targets [B, C]"
    else:
        assert targets.dtype == torch.int64 and targets.numel() == B, "kind 1: int64 labels [B]"
    dev = logits.device
    loss = torch.empty((1,), device=dev, dtype=torch.float32)
    dlogits = torch.empty((B, C), device=dev, dtype=torch.float32)
    counts = torch.empty((2,), device=dev, dtype=torch.int64)
    bad = torch.empty((1,), device=dev, dtype=torch.int32)
    call("ecamp_cls_loss", ptr(logits), ptr(targets), int(kind), ptr(loss), ptr(dlogits), ptr(counts), ptr(bad), B, C, stream())
    if check:
        cls_check_labels(bad, C)
    return loss, dlogits, counts, bad


def cls_check_labels(bad, C):
    """Raise if the flag of a `cls_loss` call says that a label lay outside [0, C).  Reads the device: call it where the loss is read."""
    if int(bad.item()) != 0:
        raise _lib.EcampHipError("cls_loss: a class label lies outside [0, %d)" % C)


def cls_head_wgrad(dlogits, feat):
    """-> (dW f32 [C, D] = dlogits^T . feat, db f32 [C] = column sums of dlogits); fixed summation order over B."""
    _chk(dlogits, feat)
    B, C = dlogits.shape
    D = feat.shape[1]
    assert dlogits.dtype == feat.dtype == torch.float32 and dlogits.is_contiguous() and feat.is_contiguous() and feat.shape[0] == B
    dw = torch.empty((C, D), device=feat.device, dtype=torch.float32)
    db = torch.empty((C,), device=feat.device, dtype=torch.float32)
    call("ecamp_cls_head_wgrad", ptr(dlogits), ptr(feat), ptr(dw), ptr(db), B, C, D, stream())
    return dw, db


# --------------------------------------------------------------------------------------------- fine-tuning (csrc/finetune.hip)
def cls_head_dgrad(dlogits, w):
    """-> dfeat f32 [B, D] = dlogits [B, C] . w [C, D]."""
    _chk(dlogits, w)
    B, C = dlogits.shape
    D = w.shape[1]
    assert dlogits.dtype == w.dtype == torch.float32 and dlogits.is_contiguous() and w.is_contiguous() and w.shape[0] == C
    dfeat = torch.empty((B, D), device=w.device, dtype=torch.float32)
    call("ecamp_cls_head_dgrad", ptr(dlogits), ptr(w), ptr(dfeat), B, C, D, stream())
    return dfeat


def pool_norm_bwd(dfeat, pooled, gamma, t0, t1, T, eps, dtype, want_affine=True):
    """Backward of `pool_norm`: dfeat / pooled f32 [B, D], gamma f32 [D] or None -> (dx [B, T, D] in `dtype`: dpooled / (t1 - t0) on the
    tokens t0 <= t < t1, zero elsewhere; dgamma, dbeta f32 [D], or None without want_affine)."""
    _chk(dfeat, pooled, gamma)
    B, D = pooled.shape
    assert dfeat.dtype == pooled.dtype == torch.float32 and dfeat.is_contiguous() and pooled.is_contiguous() and dfeat.shape == pooled.shape
    assert gamma is None or (gamma.dtype == torch.float32 and gamma.numel() == D and gamma.is_contiguous())
    dev = pooled.device
    dt = code(dtype)
    dx = torch.empty((B, T, D), device=dev, dtype=dtype)
    dgamma = torch.empty((D,), device=dev, dtype=torch.float32) if want_affine else None
    dbeta = torch.empty((D,), device=dev, dtype=torch.float32) if want_affine else None
    ws = torch.empty((max(16, int(_lib.load().ecamp_pool_norm_bwd_workspace_bytes(B, int(T), D, int(t0), int(t1), dt))),), device=dev, dtype=torch.uint8)
    call("ecamp_pool_norm_bwd", ptr(dfeat), ptr(pooled), ptr(gamma), ptr(dgamma), ptr(dbeta), ptr(dx), B, int(T), D, int(t0), int(t1), float(eps),
         ptr(ws), dt, stream())
    return dx, dgamma, dbeta


def pos_embed_grad(dx, dpos, dcls=None, dbias=None):
    """The stem's row-sum gradients from one pass over dx [B, T, D] (f32 or the active 16-bit format): with S = dx summed over the batch,
    dpos f32 [T, D] += S, dcls f32 [D] += S[0], dbias f32 [D] += S[1:] summed over the tokens.  dcls and dbias are given together or not
    at all.  Fixed summation order, no atomics; the workspace comes from the caching allocator."""
    _chk(dx, dpos, dcls, dbias)
    B, T, D = dx.shape
    assert dx.is_contiguous() and dpos.dtype == torch.float32 and dpos.is_contiguous() and dpos.numel() == T * D
    assert (dcls is None) == (dbias is None)
    for g in (dcls, dbias):
        assert g is None or (g.dtype == torch.float32 and g.is_contiguous() and g.numel() == D)
    dt = code(dx.dtype)
    ws = torch.empty((max(16, int(_lib.load().ecamp_pos_embed_grad_workspace_bytes(B, T, D, dt))),), device=dx.device, dtype=torch.uint8)
    call("ecamp_pos_embed_grad", ptr(dx), ptr(dpos), ptr(dcls), ptr(dbias), B, T, D, ptr(ws), dt, stream())


SUMSQ_MAX_SLOTS = 2048   # ecamp_sumsq_grouped fills at most this many partials per launch


def sumsq_grouped_slots(n):
    """How many f32 partials one `sumsq_grouped` launch over n elements fills (a function of n alone)."""
    return int(_lib.load().ecamp_sumsq_grouped_slots(int(n)))


def sumsq_grouped(g, block_group, partials):
    """sum(g^2) over the 64-element blocks of the flat f32 `g` whose `block_group` byte is below 8, one partial per workgroup into
    `partials[0:slots]` (a slice of a larger buffer is fine) -> slots.  No scalar: `sgd_grouped` adds the partials itself."""
    _chk(g, block_group, partials)
    n = g.numel()
    assert g.dtype == torch.float32 and g.is_contiguous() and block_group.dtype == torch.uint8 and block_group.numel() == n // 64
    slots = sumsq_grouped_slots(n)
    assert partials.dtype == torch.float32 and partials.is_contiguous() and (slots == 0 or partials.numel() >= slots)
    call("ecamp_sumsq_grouped", ptr(g), ptr(block_group), n, ptr(partials), None, stream())
    return slots


def sgd_grouped(p, g, buf, p16, block_group, lrs, wds, momentum, max_norm, partials, npart, grad_scale=1.0, ctl=None, norm_out=None):
    """clip_grad_norm_(max_norm) + torch.optim.SGD(momentum) over a flat buffer (include/ecamp_hip.h): `partials[0:npart]` are the
    sums of squares of the (scaled) gradients, `ctl` the optional device f32[4] of `loss_scale_update`, `norm_out` an optional device
    f32[1] for the global norm."""
    _chk(p, g, buf, p16, block_group, partials, ctl, norm_out)
    n = len(lrs)
    arr = ctypes.c_float * n
    call("ecamp_sgd_grouped", ptr(p), ptr(g), ptr(buf), ptr(p16), ptr(block_group), p.numel(), n, arr(*lrs), arr(*wds), float(momentum),
         float(max_norm), ptr(partials), int(npart), float(grad_scale), ptr(ctl), ptr(norm_out), stream())


def sgd_scale_update(partials, npart, state, ctl, norm_out, growth, backoff, window, max_scale):
    """apex's dynamic loss-scale rule around `sgd_grouped`, decided on the device (include/ecamp_hip.h): `partials[0:npart]` are the sums of
    squares of the SCALED gradients, `state` the device f32[4] {scale, clean steps, skipped, skipped in a row}, `ctl` the device f32[4]
    `sgd_grouped` then reads, `norm_out` an optional device f32[1] for the norm of the un-scaled gradients.  Nothing is read back."""
    _chk(partials, state, ctl, norm_out)
    call("ecamp_sgd_scale_update", ptr(partials), int(npart), ptr(state), ptr(ctl), ptr(norm_out), float(growth), float(backoff), int(window),
         float(max_scale), stream())


# --------------------------------------------------------------------------------------------- optimizer side
def sumsq(x, out):
    call("ecamp_sumsq", ptr(x), x.numel(), ptr(out), stream())


def adamw(p, g, m, v, p16, lr, beta1, beta2, eps, wd, step, grad_scale=1.0):
    call("ecamp_adamw", ptr(p), ptr(g), ptr(m), ptr(v), ptr(p16), p.numel(), float(lr), float(beta1), float(beta2), float(eps),
         float(wd), int(step), float(grad_scale), stream())


def adamw_grouped(p, g, m, v, p16, block_group, lrs, wds, beta1, beta2, eps, step, grad_scale=1.0, grad_sumsq=None, ctl=None):
    """grad_sumsq: optional zeroed f32[1]; receives sum((g * grad_scale)^2) over the updated elements (global grad-norm, fused).
    ctl: optional device f32[4] from loss_scale_update -- grad scale, skip flag and bias corrections are then read on the device."""
    n = len(lrs)
    arr = ctypes.c_float * n
    call("ecamp_adamw_grouped", ptr(p), ptr(g), ptr(m), ptr(v), ptr(p16), ptr(block_group), p.numel(), n, arr(*lrs), arr(*wds),
         float(beta1), float(beta2), float(eps), int(step), float(grad_scale), ptr(grad_sumsq), ptr(ctl), stream())


def loss_scale_update(sumsq_, state, opt_step, ctl, norm_out, growth, backoff, interval, beta1, beta2):
    """GradScaler's unscale_ / step / update on the device (no host read): see include/ecamp_hip.h."""
    _chk(sumsq_, state, opt_step, ctl)
    call("ecamp_loss_scale_update", ptr(sumsq_), ptr(state), ptr(opt_step), ptr(ctl), ptr(norm_out), float(growth), float(backoff), int(interval),
         float(beta1), float(beta2), stream())


# --------------------------------------------------------------------------------------------- side-stream weight gradients
# Weight gradients are leaves of the backward dependency graph: nothing in backward waits for them.  Launching them on a
# second HIP stream lets their workgroups fill the tail-quantisation gaps of the dgrad / attention / LayerNorm kernels on the
# main stream (and vice versa).  The main stream re-joins at the end of backward (streams.on_wgrad_stream: stream, held operands, join).
OVERLAP_WGRAD = os.environ.get("ECAMP_OVERLAP_WGRAD", "1") != "0"

# The image decoder + pixel losses and the report side both hang off the encoder's latent and nothing else: run on two streams,
# the workgroups of one fill the tail rounds of the other's persistent GEMMs (forward AND backward: autograd replays each
# stage's backward on the stream its forward ran on).  Measured on MI355X at B=256, same-box A/B of 30-step runs on three boxes
# (round 3, after the phase-schedule GEMM and the one-launch-per-block weight gradients): step 37.4-37.5 -> 36.6-36.65 ms, forward
# 14.3 -> 14.0, forward+backward 35.9 -> 35.1 (in round 2 the same switch bought 0.15 ms: the slower GEMMs left fewer gaps that
# the weight-gradient stream did not already fill).  On by default; ECAMP_OVERLAP_BRANCHES=0 serialises the two branches
# (ECAMP.forward: streams.fork_branch / join_branch).
OVERLAP_BRANCHES = os.environ.get("ECAMP_OVERLAP_BRANCHES", "1") != "0"


def wgrad_group_async(items, workgroups=0):
    """wgrad_group on the weight-gradient stream (see linear_wgrad_async)."""
    if not OVERLAP_WGRAD:
        return wgrad_group(items, workgroups=workgroups)
    streams.on_wgrad_stream(items[0][0].device, lambda: wgrad_group(items, workgroups=workgroups), [(dy, x) for dy, x, _, _, _ in items])


def linear_wgrad_async(dy, x, gw, alpha=1.0, alpha_dev=None, gb=None, accumulate=True):
    if not OVERLAP_WGRAD:
        return linear_wgrad(dy, x, gw, alpha, alpha_dev, gb, accumulate)
    streams.on_wgrad_stream(dy.device, lambda: linear_wgrad(dy, x, gw, alpha, alpha_dev, gb, accumulate), [(dy, x, alpha_dev)])


# --------------------------------------------------------------------------------------------- dataset image transform on the device
def resample_crops_workspace_bytes(B, out, kmax, tmp_rows):
    return int(_lib.load().ecamp_resample_crops_workspace_bytes(int(B), int(out), int(kmax), int(tmp_rows)))


def resample_boxes_workspace_bytes(B, out, kmax, tmp_rows):
    return int(_lib.load().ecamp_resample_boxes_workspace_bytes(int(B), int(out), int(kmax), int(tmp_rows)))


BILINEAR, BICUBIC = 0, 1   # the `filter` argument of ecamp_resample_boxes_u8


def _resample(name, width, flat, table, out_t, out, kmax, tmp_rows, max_h, ws, err, *filter):
    """The one body of the three resample entry points: `width` is the table's, `filter` is given where the entry point takes one."""
    _chk(flat, table, out_t, ws, err)
    assert flat.dtype == torch.uint8 and table.dtype == torch.int64 and table.is_contiguous() and table.shape[1] == width
    assert out_t.dtype == torch.uint8 and out_t.is_contiguous() and tuple(out_t.shape) == (table.shape[0], out, out)
    call(name, ptr(flat), ptr(table), ptr(out_t), table.shape[0], int(out), int(kmax), int(tmp_rows), int(max_h), *map(int, filter), ptr(ws), ws.numel(), ptr(err),
         stream())
    return out_t


def resample_crops_u8(flat, table, out_t, out, kmax, tmp_rows, max_h, ws, err):
    """B crops (flat uint8 + int64 table [B, 6], both on the device) -> out_t uint8 [B, out, out]: Pillow's crop().resize(BICUBIC) + flip,
    byte for byte (csrc/augment.hip; pretrain_datasets.py:47-52)."""
    return _resample("ecamp_resample_crops_u8", 6, flat, table, out_t, out, kmax, tmp_rows, max_h, ws, err)


def resample_boxes_u8(flat, table, out_t, out, kmax, tmp_rows, max_h, ws, err, filter=BILINEAR):
    """B boxes (flat uint8 + int64 table [B, 10]: off, h, w, flip, row0, full_w, shift_w, full_h, shift_h, 0; both on the device) -> out_t
    uint8 [B, out, out]: Pillow's resize of every axis to `full` (BILINEAR or BICUBIC), the `out` pixels from `shift` on, zero outside, +
    flip -- byte for byte the classification transforms (csrc/augment.hip; module/finetune_datasets.py)."""
    return _resample("ecamp_resample_boxes_u8", 10, flat, table, out_t, out, kmax, tmp_rows, max_h, ws, err, filter)


def resample_boxes_rgb_u8(flat, table, out_t, out, kmax, tmp_rows, max_h, ws, err, filter=BILINEAR):
    """`resample_boxes_u8` for batches with colour samples: table column 9 is the plane count c (3: planar R, G, B, 3 x h x w bytes at off and
    3 h intermediate rows from row0; else one plane), tmp_rows / max_h count c * h.  Three planes through the same taps, then Pillow's
    convert("L") -- byte for byte Grayscale after the resize of the RGB image; a one-plane sample gets `resample_boxes_u8`'s byte."""
    return _resample("ecamp_resample_boxes_rgb_u8", 10, flat, table, out_t, out, kmax, tmp_rows, max_h, ws, err, filter)


def resample_shard_u8(shard, table, out_t, out, kmax, tmp_rows, max_h, ws, err, filter=BILINEAR):
    """`resample_boxes_rgb_u8` on a shard that stays in device memory: `shard` is the whole uploaded file (flat uint8), table int64 [B, 12] =
    the stride-10 row + (pitch, plane_pitch) of the stored image, `off` the byte offset in `shard` of the box's first pixel -- the boxes are
    read where they lie.  A row that points outside `shard` gives a sample of zeros and ORs 2 into `err` (1: more than `kmax` taps)."""
    _chk(shard, table, out_t, ws, err)
    assert shard.dtype == torch.uint8 and shard.dim() == 1 and shard.is_contiguous()
    assert table.dtype == torch.int64 and table.is_contiguous() and table.shape[1] == 12
    assert out_t.dtype == torch.uint8 and out_t.is_contiguous() and tuple(out_t.shape) == (table.shape[0], out, out)
    call("ecamp_resample_shard_u8", ptr(shard), shard.numel(), ptr(table), ptr(out_t), table.shape[0], int(out), int(kmax), int(tmp_rows), int(max_h), int(filter),
         ptr(ws), ws.numel(), ptr(err), stream())
    return out_t
