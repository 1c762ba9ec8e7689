"""The attention kernels of csrc/attention.hip and csrc/attention_bf16.hip in plain torch on the CPU: what tests/test_attn_float64_gpu.py
holds ecamp_attn_fwd / ecamp_attn_bwd / ecamp_attn_probs to, element by element, and what tests/test_attn_reference_cpu.py proves about
it without a GPU.  Method and vocabulary are those of tests/_sr_ref.py, _report_ref.py and _gemm_ref.py, whose U, TINY, stored, k_of,
bound_k, R and PATTERN are used as they are.

Everything is float64 on the values the kernel is given, [B, H, T, hd] per operand.
  forward   s = scale q.k     P = softmax over the attended keys     Pd = P keep / (1 - p)     O = Pd v     lse = ln sum_j exp s_ij
            keep = hip_ops.dropout_mask at element index ((b H + h) Tq + i) Tk + j (ones without dropout); scale and p are the float32
            values the C ABI receives.
  backward  judged on what it is HANDED, the O and lse the forward call stored (that call is judged first, and it is the only way to
            saved dropout bits):  P = exp(s - lse)   delta = sum_d dO O   dP = dO.v   dS = P (dP keep/(1-p) - delta)
            dV = Pd^T dO   dQ = scale dS k   dK = scale dS^T q
Magnitudes: the same arithmetic on absolute values with no minus sign.  As = scale |q|.|k|, W_i = sum_l P_il As_il, F_ij = As_ij + W_i
(what a relative f32-unit error of the scores does to P_ij through the softmax, to first order), A_dS = P (|dO|.|v| keep/(1-p) +
sum_d |dO| |O|).  Every judged quantity has two parts, each with its own unit:
      quantity   format part (unit R[fmt])        f32 part (unit U32)
      O          sum_j Pd |v|                     sum_j Pd F |v|
      dV         sum_i Pd |dO|                    sum_i Pd F |dO|
      dQ         scale sum_j A_dS |k|             scale sum_j A_dS F |k|
      dK         scale sum_i A_dS |q|             scale sum_i A_dS F |q|
      lse        -                                |lse| + 1 + W
      probs      -                                P F                       (ecamp_attn_probs, f32 output)
  the format part covers P keep (dS) rounded ONCE to the 16-bit format as a matrix-core operand plus the stored output (each half an R);
  with f32 operands every unit is the f32 one (R[F32] = U32).
Bound, EVERY element:   |got - ref| <= K (R[fmt] A_fmt + U32 A_32) + tiny,   K = bound_k(K_yard) = max(1, 4 K_yard)
  tiny: TINY[fmt] for the stored value plus TINY[fmt] times the sum of the other operand's magnitudes (sum_j |v| keep/(1-p) for O, ...):
  a P or dS entry that falls into the format's subnormal range is off by up to half a subnormal step whatever its size (bfloat16: nothing,
  half: 2^-25 per entry).  It applies only where A > 0.
Structural zeros: where A == 0 the bound is 0 and the element must BE zero -- dK / dV rows of keys behind the mask, every probability
  behind the mask, the O / dQ row of a query whose every attended key was dropped.  Nothing is excluded from any judgement.
Yardstick: the same arithmetic in float32, every contraction a chain in index order (one product per step, never torch.matmul, which sums
  blockwise), the softmax as max / exp / sum; P keep and dS rounded once to the 16-bit format where the kernels pack their MFMA operands,
  outputs rounded once to the storage format.  K_yard = its largest (err - tiny) / (R A_fmt + U32 A_32); K is computed per case and
  quantity from it, never written down and never taken from a kernel's result.

Regimes: plain (randn), peaked (q x 4: near one-hot rows, dS cancels heavily), pad40 (keys behind the mask carry 40 x the scale: the half
  NaN regression of test_attention_padded_keys_with_large_scores_stay_out_of_the_gradients, with exact-zero dK / dV rows).  Draws are
  floored to |x| >= 2^-8: subnormal OPERANDS are out of scope.  Key lengths of a masked case: Tk, Tk // 2 + 3, 5 for B = 3, the first two
  for B = 2, Tk // 2 + 3 for B = 1.  Every batch attends at least one key: a fully masked batch is outside the kernels' contract
  (attn_head_fwd_kernel writes O = 0 and lse = -inf there) and out of scope, as are head widths other than 32 / 64 / 128 and the
  ECAMP_ATTN_WAVES override.

Selection: select() restates attn_select / attn16_select / head_lds_bytes / attn_kch and the workgroup size of csrc/attention*.h(ip) in
  plain arithmetic; GPU_CASES carries, written by hand, the (family, kch, FLAGS, bits, waves) every GPU case is meant to reach in its
  forward and its backward call, and tag_of the profiler tag that proves it
      attn:<family>:<f|b>:<hd>:<Tq>:<Tk>:k<kch>F<FLAGS>b<bits>w<waves>.

Buffers (Tokens): the three production layouts of ecamp_amd/functions.py -- `packed` (ViT [B,T,3,H,hd] and BERT [B,S,3H] address alike:
  q, k, v at columns 0, D, 2D of one token row; T = max(Tq, Tk), rows past an operand's own length are not its) and `cross` (q dense, k / v
  in [B,Tk+1,2D] from token 1).  Token stride width + 8, 8 guard token rows before the first batch, after every batch; input pads, guards,
  foreign rows and the cross buffer's token 0 hold NaN, outputs 0x5A5A5A5A everywhere.  `dense`: no pad, no rows between batches."""
import collections

import torch

from _gemm_ref import PATTERN, R
from _report_ref import BF16, DTYPE, F16, F32, TINY, U, stored  # noqa: F401
from _sr_ref import bound_k, k_of  # noqa: F401

U32 = U[F32]
FLOOR = 2.0 ** -8
PAD, GUARD = 8, 8
LDS_MAX = 160 * 1024
OLD_TOL = {F32: 2e-5, BF16: 2e-2, F16: 3e-3}       # check() of tests/test_kernels_gpu.py: max|got - ref| / max|ref|, doubled for gradients
REGIMES = ("plain", "peaked", "pad40")
SEED, OFFSET = 0x1234ABCD5678, 41                  # the Philox pair of every GPU call


# ================================================================================================ the kernel selection, restated
def attn_kch(Tk):
    return 1 if Tk <= 64 else 2 if Tk <= 128 else 4 if Tk <= 256 else 0


def head_lds_bytes(Tq, Tk, hd, backward, bits):
    nkp, nqp = ((Tk + 15) // 16 + 1) // 2, ((Tq + 15) // 16 + 1) // 2
    prow = (nqp if backward and nqp > nkp else nkp) * 32
    return 2 * prow * 2 * hd + (3 if backward else 1) * prow * 4 + (32 * prow if backward and bits else 0)


def mask_bytes(B, H, Tq, Tk, hd, fmt, head=1):
    """ecamp_attn_mask_bytes: the size of the saved dropout bits, 0 where the forward call is not head-resident."""
    if fmt == F32 or Tk > 256 or head == 0 or head_lds_bytes(Tq, Tk, hd, False, False) > LDS_MAX:
        return 0
    return B * H * Tq * 32


Sel = collections.namedtuple("Sel", "family kch flags bits waves")


def select(fmt, Tq, Tk, hd, flags, bits, backward, head=1):
    """attn_select -> Sel.  flags: key mask or dropout; bits: a dropout-bits buffer reaches the call; head: the attn_head switch (0 = off)."""
    flags = int(bool(flags))
    if fmt == F32:
        return Sel("f32", attn_kch(Tk), flags, 0, 4)
    nqt, nkt = (Tq + 15) // 16, (Tk + 15) // 16
    if head != 0 and head_lds_bytes(Tq, Tk, hd, backward, bits) <= LDS_MAX:
        return Sel("head", None, flags, int(bool(bits)), min(max(nkt, nqt), 4) if backward else min(nqt, 8))
    if backward:
        return Sel("stream", attn_kch(Tk), flags, 0, 4)
    if Tk > 128:
        return Sel("long", None, flags, 0, 4)
    return Sel("resident", attn_kch(Tk), flags, 0, 4)


def tag_of(sel, backward, hd, Tq, Tk):
    return "attn:%s:%s:%d:%d:%d:k%sF%db%dw%d" % (sel.family, "b" if backward else "f", hd, Tq, Tk, "-" if sel.kch is None else sel.kch,
                                                 sel.flags, sel.bits, sel.waves)


# ---- the GPU cases and the kernel every call of them is MEANT to reach, written down by hand
# id: (layout, (B, H, Tq, Tk, hd), masked, p, attn_head switch, forward, backward given the bits, backward regenerating the mask)
_H, _S = "head", "stream"
GPU_CASES = {
    # head-resident, FLAGS 0
    "h0-17":      ("packed", (1, 2, 17, 17, 32), False, 0.0, -1, (_H, None, 0, 0, 2), None, (_H, None, 0, 0, 2)),
    "h0-50":      ("packed", (2, 3, 50, 50, 32), False, 0.0, -1, (_H, None, 0, 0, 4), None, (_H, None, 0, 0, 4)),
    "h0-64":      ("packed", (2, 2, 64, 64, 128), False, 0.0, -1, (_H, None, 0, 0, 4), None, (_H, None, 0, 0, 4)),
    "h0-197":     ("packed", (2, 2, 197, 197, 64), False, 0.0, -1, (_H, None, 0, 0, 8), None, (_H, None, 0, 0, 4)),
    "h0-x288":    ("cross", (1, 2, 40, 288, 128), False, 0.0, -1, (_H, None, 0, 0, 3), None, (_H, None, 0, 0, 4)),
    # head-resident, FLAGS 1: key mask, without and with dropout
    "h1-17":      ("packed", (3, 2, 33, 17, 32), True, 0.0, -1, (_H, None, 1, 0, 3), None, (_H, None, 1, 0, 3)),
    "h1-17-p":    ("packed", (3, 2, 33, 17, 32), True, 0.3, -1, (_H, None, 1, 1, 3), (_H, None, 1, 1, 3), (_H, None, 1, 0, 3)),
    "h1-100":     ("packed", (3, 2, 100, 100, 64), True, 0.0, -1, (_H, None, 1, 0, 7), None, (_H, None, 1, 0, 4)),
    "h1-100-p":   ("packed", (3, 2, 100, 100, 64), True, 0.1, -1, (_H, None, 1, 1, 7), (_H, None, 1, 1, 4), (_H, None, 1, 0, 4)),
    "h1-48":      ("packed", (3, 2, 48, 48, 64), True, 0.0, -1, (_H, None, 1, 0, 3), None, (_H, None, 1, 0, 3)),
    "h1-48-p":    ("packed", (3, 2, 48, 48, 64), True, 0.1, -1, (_H, None, 1, 1, 3), (_H, None, 1, 1, 3), (_H, None, 1, 0, 3)),
    "h1-128":     ("packed", (3, 2, 128, 128, 128), True, 0.0, -1, (_H, None, 1, 0, 8), None, (_H, None, 1, 0, 4)),
    "h1-128-p":   ("packed", (3, 2, 128, 128, 128), True, 0.1, -1, (_H, None, 1, 1, 8), (_H, None, 1, 1, 4), (_H, None, 1, 0, 4)),
    # cross layout
    "x-128-49-p": ("cross", (2, 2, 128, 49, 128), False, 0.1, -1, (_H, None, 1, 1, 8), (_H, None, 1, 1, 4), (_H, None, 1, 0, 4)),
    "x-40-49":    ("cross", (2, 2, 40, 49, 128), False, 0.0, -1, (_H, None, 0, 0, 3), None, (_H, None, 0, 0, 4)),
    "x-20-150":   ("cross", (2, 2, 20, 150, 64), False, 0.0, -1, (_H, None, 0, 0, 2), None, (_H, None, 0, 0, 4)),
    "x-150-20":   ("cross", (2, 2, 150, 20, 64), False, 0.0, -1, (_H, None, 0, 0, 8), None, (_H, None, 0, 0, 4)),
    # head forward writes bits; the backward image (320 rows of 128) does not fit LDS with or without them: streaming pair, mask regenerated
    "x-300-70-p": ("cross", (1, 2, 300, 70, 128), False, 0.1, -1, (_H, None, 1, 1, 8), (_S, 2, 1, 0, 4), (_S, 2, 1, 0, 4)),
    # attn_head = 0
    "s-50":       ("packed", (2, 2, 50, 50, 64), False, 0.0, 0, ("resident", 1, 0, 0, 4), None, (_S, 1, 0, 0, 4)),
    "s-100-p":    ("packed", (3, 2, 100, 100, 32), True, 0.1, 0, ("resident", 2, 1, 0, 4), None, (_S, 2, 1, 0, 4)),
    "s-70-130":   ("packed", (1, 2, 70, 130, 128), False, 0.0, 0, ("long", None, 0, 0, 4), None, (_S, 4, 0, 0, 4)),
    "s-130-200-p": ("packed", (1, 2, 130, 200, 64), True, 0.1, 0, ("long", None, 1, 0, 4), None, (_S, 4, 1, 0, 4)),
    "s-70-300":   ("packed", (1, 2, 70, 300, 128), True, 0.0, 0, ("long", None, 1, 0, 4), None, (_S, 0, 1, 0, 4)),
    "d-70-300":   ("packed", (1, 2, 70, 300, 128), True, 0.0, -1, ("long", None, 1, 0, 4), None, (_S, 0, 1, 0, 4)),      # default switches: too long for a head
}
F32_CASES = {
    "f-50":       ("packed", (2, 2, 50, 50, 64), False, 0.0, -1, ("f32", 1, 0, 0, 4), None, ("f32", 1, 0, 0, 4)),
    "f-100-p":    ("packed", (3, 2, 100, 100, 32), True, 0.1, -1, ("f32", 2, 1, 0, 4), None, ("f32", 2, 1, 0, 4)),
    "f-70-200":   ("packed", (1, 2, 70, 200, 128), False, 0.0, -1, ("f32", 4, 0, 0, 4), None, ("f32", 4, 0, 0, 4)),
    "f-x40-49":   ("cross", (2, 2, 40, 49, 128), False, 0.0, -1, ("f32", 1, 0, 0, 4), None, ("f32", 1, 0, 0, 4)),
    "f-70-300":   ("packed", (1, 2, 70, 300, 64), True, 0.0, -1, ("f32", 0, 1, 0, 4), None, ("f32", 0, 1, 0, 4)),        # one wave per row
}
# regime coverage beyond `plain` (which every case runs): peaked on one case per family and pass, pad40 on the masked FLAGS 1 cases and
# one streaming case
PEAKED = ("h0-50", "h1-100-p", "x-300-70-p", "s-100-p", "s-130-200-p", "f-100-p")
PAD40 = ("h1-17-p", "h1-100-p", "h1-48-p", "h1-128-p", "h1-128", "s-100-p", "f-100-p")
DENSE = ("h0-50", "h1-48-p", "x-40-49", "s-50", "s-130-200-p", "f-50")      # one dense (wrap-around) call per family
PROBS_CASES = {"p-40-49": ((2, 2, 40, 49, 128), False), "p-33-300": ((2, 2, 33, 300, 32), True)}


def gpu_runs():
    """(case id, regime) of every 16-bit GPU run, then of every f32 one."""
    half = [(i, r) for i in GPU_CASES for r in REGIMES if r == "plain" or (r == "peaked" and i in PEAKED) or (r == "pad40" and i in PAD40)]
    f32 = [(i, r) for i in F32_CASES for r in REGIMES if r == "plain" or (r == "peaked" and i in PEAKED) or (r == "pad40" and i in PAD40)]
    return half, f32


def intended(case_id):
    layout, shape, masked, p, head, fwd, bwd_bits, bwd_regen = {**GPU_CASES, **F32_CASES}[case_id]
    return layout, shape, masked, p, head, Sel(*fwd), None if bwd_bits is None else Sel(*bwd_bits), Sel(*bwd_regen)


# ================================================================================================ inputs
def key_lengths(B, Tk):
    return {1: [Tk // 2 + 3], 2: [Tk, Tk // 2 + 3], 3: [Tk, Tk // 2 + 3, 5]}[B]


def _draw(g, *shape):
    t = torch.randn(*shape, generator=g)
    return torch.where(t.abs() < FLOOR, torch.copysign(torch.full_like(t, FLOOR), t), t)


def _round_bits(x, bits):
    """x rounded to `bits` significant bits."""
    m, e = torch.frexp(x)
    return torch.ldexp(torch.round(m * 2.0 ** bits) / 2.0 ** bits, e)


Quantity = collections.namedtuple("Quantity", "ref Afmt A32 tiny fmt")      # fmt: the storage format of the output


def unit_bound(q, fmt):
    """R A_fmt + U32 A_32: the bound at K = 1 without the tiny term.  fmt: the operand format."""
    return R[fmt] * q.Afmt + U32 * q.A32


def bound(q, fmt, K):
    ub = unit_bound(q, fmt)
    return K * ub + q.tiny * (ub > 0)


class Case:
    """One (format, shape, regime, mask, dropout) on the host: inputs as [B, H, T, hd] float32 tensors exact in the format, the float64
    reference with its magnitudes, the float32 yardstick and the mutants."""

    def __init__(self, fmt, B, H, Tq, Tk, hd, regime="plain", masked=False, p=0.0):
        assert regime in REGIMES and hd in (32, 64, 128) and (masked or regime != "pad40")
        self.fmt, self.B, self.H, self.Tq, self.Tk, self.hd, self.regime, self.masked, self.p = fmt, B, H, Tq, Tk, hd, regime, masked, p
        g = torch.Generator().manual_seed(1000003 * REGIMES.index(regime) + 7919 * Tq + 31 * Tk + 17 * hd + 5 * B + H)
        q, k, v, do = _draw(g, B, H, Tq, hd), _draw(g, B, H, Tk, hd), _draw(g, B, H, Tk, hd), _draw(g, B, H, Tq, hd)
        if regime == "peaked":
            q = q * 4.0
        self.lens = key_lengths(B, Tk) if masked else [Tk] * B
        assert min(self.lens) >= 1, "a fully masked batch is out of scope"
        self.key_mask = (torch.arange(Tk)[None, :] < torch.tensor(self.lens)[:, None]).to(torch.int32) if masked else None
        self.att = (torch.arange(Tk)[None, :] < torch.tensor(self.lens)[:, None])[:, None, None, :]      # [B, 1, 1, Tk] bool
        if regime == "pad40":
            k = torch.where(self.att.transpose(-1, -2), k, k * 40.0)
        self.q, self.k, self.v, self.do = (stored(t, fmt) for t in (q, k, v, do))
        self.scale = float(torch.tensor(hd ** -0.5, dtype=torch.float32))
        self.p32 = float(torch.tensor(p, dtype=torch.float32))
        self.ik = 1.0 / (1.0 - self.p32)
        self._s = None

    def name(self):
        return "%-4s (%d,%d,%d,%d,%d) %-6s mask %d p %.1f" % (self.fmt, self.B, self.H, self.Tq, self.Tk, self.hd, self.regime, self.masked, self.p)

    def ones(self):
        return torch.ones(self.B, self.H, self.Tq, self.Tk)

    def host_keep(self, seed=0):
        """A keep-mask for the tests that have no GPU to ask (any 0 / 1 tensor is a legal input of the reference)."""
        if self.p == 0:
            return self.ones()
        g = torch.Generator().manual_seed(99 + seed)
        return (torch.rand(self.B, self.H, self.Tq, self.Tk, generator=g) >= self.p).float()

    # ------------------------------------------------------------------------------------------------ the arithmetic, once
    def _mm(self, a, b, yard):
        """a [.., M, K] @ b [.., K, N]; the yardstick's is a float32 chain in k order, one product per step."""
        if not yard:
            return a @ b
        acc = torch.zeros(a.shape[:-1] + b.shape[-1:], dtype=torch.float32)
        for kk in range(a.shape[-1]):
            acc = acc + a[..., :, kk:kk + 1] * b[..., kk:kk + 1, :]
        return acc

    def _pack(self, t, yard):
        """Where the kernels round an MFMA operand to the 16-bit format."""
        return stored(t, self.fmt) if (yard and self.fmt != F32) else t

    def _out(self, t):
        return stored(t.float(), self.fmt)

    def _fwd(self, keep, yard=False, mut=None):
        """-> (O as stored, lse float32, P of the arithmetic's own type)."""
        dt = torch.float32 if yard else torch.float64
        q, k, v, keep = self.q.to(dt), self.k.to(dt), self.v.to(dt), keep.to(dt)
        scale = self.scale * (1.0 + 2.0 ** -9 if mut == "scale" else 1.0)
        s = (self._mm(q, k.transpose(-1, -2), yard) * scale).masked_fill(~self.att, float("-inf"))
        m = s.max(-1, keepdim=True).values
        e = torch.exp(s - m)
        l = e.sum(-1, keepdim=True)
        if mut == "rowsum":            # the last attended key is left out of the row sum of the last query tile
            i0 = 16 * ((self.Tq - 1) // 16)
            last = torch.tensor(self.lens)[:, None, None, None].expand(self.B, self.H, self.Tq, 1) - 1
            l = l.clone()
            l[:, :, i0:] -= e.gather(-1, last)[:, :, i0:]
        lse = m + torch.log(l)
        P = e / l
        ik = torch.full((self.Tk,), self.ik, dtype=dt)
        if mut == "inv_keep":          # 1 / (1 - p) missing on the last 32-key pair
            ik[32 * ((self.Tk - 1) // 32):] = 1.0
        O = self._mm(self._pack(P * keep, yard) * ik, v, yard)
        if mut == "row":               # the last query row written from its neighbour
            O = O.clone()
            O[:, :, -1] = O[:, :, -2]
        return self._out(O), lse[..., 0].float(), P

    def forward(self, keep):
        """The float64 reference of the forward call -> {"O": Quantity, "lse": Quantity} (and what the backward magnitudes reuse)."""
        q, k, v, keep = self.q.double(), self.k.double(), self.v.double(), keep.double()
        s = (q @ k.transpose(-1, -2) * self.scale).masked_fill(~self.att, float("-inf"))
        As = q.abs() @ k.abs().transpose(-1, -2) * self.scale
        lse = torch.logsumexp(s, -1, keepdim=True)
        P = torch.exp(s - lse)
        assert bool((P.masked_select(~self.att.expand_as(P)) == 0).all())
        W = (P * As).sum(-1, keepdim=True)
        F = As + W
        Pd = P * keep * self.ik
        tiny = TINY[self.fmt] * ((keep * self.ik * self.att) @ v.abs() + 1.0)
        out = {"O": Quantity(Pd @ v, Pd @ v.abs(), (Pd * F) @ v.abs(), tiny, self.fmt),
               "lse": Quantity(lse[..., 0], torch.zeros_like(lse[..., 0]), (lse.abs() + 1.0 + W)[..., 0], TINY[F32], F32)}
        self._s, self._As = s, As
        return out

    def probs(self):
        """ecamp_attn_probs: P itself, f32, judged with the f32 part alone; exactly 0 behind the mask."""
        q, k = self.q.double(), self.k.double()
        s = (q @ k.transpose(-1, -2) * self.scale).masked_fill(~self.att, float("-inf"))
        As = q.abs() @ k.abs().transpose(-1, -2) * self.scale
        P = torch.softmax(s, -1)
        F = As + (P * As).sum(-1, keepdim=True)
        return {"probs": Quantity(P, torch.zeros_like(P), P * F, TINY[F32], F32)}

    def probs_yard(self):
        return {"probs": self._fwd(self.ones(), yard=True)[2]}

    def _bwd(self, O_given, lse_given, keep, yard=False, mut=None):
        """-> (dQ, dK, dV) as stored."""
        dt = torch.float32 if yard else torch.float64
        q, k, v, do, keep = self.q.to(dt), self.k.to(dt), self.v.to(dt), self.do.to(dt), keep.to(dt)
        Og, lse = O_given.to(dt), lse_given.to(dt).clone()
        s = self._mm(q, k.transpose(-1, -2), yard) * self.scale
        if mut == "lse":               # one query row of the second trip uses the lse of the row 128 above it
            i = 128 + int((lse[0, 0, 128:] - lse[0, 0, :self.Tq - 128]).abs().argmax())
            lse[0, 0, i] = lse[0, 0, i - 128]
        Pun = torch.exp(s - lse[..., None])
        P = Pun.masked_fill(~self.att, 0.0)
        if mut == "delta":             # delta taken from an O that went through a second, 16-bit rounding
            Og = _round_bits(Og, {F32: 8, BF16: 7, F16: 10}[self.fmt])
        delta = (do * Og).sum(-1, keepdim=True)
        dP = self._mm(do, v.transpose(-1, -2), yard)
        dS = self._pack(P * (dP * (keep * self.ik) - delta), yard)
        Pd = self._pack(P * keep, yard) * self.ik
        dV = self._mm(Pd.transpose(-1, -2), do, yard)
        dQ = self._mm(dS, k, yard) * self.scale
        dK = self._mm(dS.transpose(-1, -2), q, yard) * self.scale
        if mut == "dv_leak":           # a masked key's dV row is 1e-6 times its unmasked value
            leak = 1e-6 * ((Pun * keep * self.ik).transpose(-1, -2) @ do)
            dV = torch.where(self.att.transpose(-1, -2), dV, leak)
        if mut == "dk_scale":          # dK of one 16-key tile missing `scale`
            dK = dK.clone()
            dK[:, :, 16:32] /= self.scale
        return self._out(dQ), self._out(dK), self._out(dV)

    def backward(self, O_given, lse_given, keep):
        """The float64 reference of the backward call on the O and lse it is handed -> {"dQ", "dK", "dV": Quantity}."""
        q, k, v, do, keep = self.q.double(), self.k.double(), self.v.double(), self.do.double(), keep.double()
        Og, lse = O_given.double(), lse_given.double()[..., None]
        s = q @ k.transpose(-1, -2) * self.scale
        As = q.abs() @ k.abs().transpose(-1, -2) * self.scale
        P = torch.exp(s - lse).masked_fill(~self.att, 0.0)
        F = As + (P * As).sum(-1, keepdim=True)
        kk = keep * self.ik
        delta, Adelta = (do * Og).sum(-1, keepdim=True), (do.abs() * Og.abs()).sum(-1, keepdim=True)
        dP, AdP = do @ v.transpose(-1, -2), do.abs() @ v.abs().transpose(-1, -2)
        dS, AdS = P * (dP * kk - delta), P * (AdP * kk + Adelta)
        Pd = P * kk
        T = lambda t: t.transpose(-1, -2)      # noqa: E731
        att = self.att.double()
        tq = TINY[self.fmt] * (self.scale * (att @ k.abs()) + 1.0)                                  # [B, H, 1, hd]
        tk = TINY[self.fmt] * (self.scale * q.abs().sum(-2, keepdim=True) + 1.0)
        tv = TINY[self.fmt] * (self.ik * do.abs().sum(-2, keepdim=True) + 1.0)
        sc = self.scale
        return {"dQ": Quantity(sc * dS @ k, sc * AdS @ k.abs(), sc * (AdS * F) @ k.abs(), tq.expand(-1, -1, self.Tq, -1), self.fmt),
                "dK": Quantity(sc * T(dS) @ q, sc * T(AdS) @ q.abs(), sc * T(AdS * F) @ q.abs(), tk.expand(-1, -1, self.Tk, -1), self.fmt),
                "dV": Quantity(T(Pd) @ do, T(Pd) @ do.abs(), T(Pd * F) @ do.abs(), tv.expand(-1, -1, self.Tk, -1), self.fmt)}

    # ------------------------------------------------------------------------------------------------ what a kernel could return
    def fwd_outputs(self, keep, yard=False, mut=None):
        O, lse, _ = self._fwd(keep, yard, mut)
        return {"O": O, "lse": lse}

    def bwd_outputs(self, O_given, lse_given, keep, yard=False, mut=None):
        return dict(zip(("dQ", "dK", "dV"), self._bwd(O_given, lse_given, keep, yard, mut)))


# ================================================================================================ the judge
def k_yard_of(case, ref, yard):
    """{quantity: K_yard}: the yardstick's largest (err - tiny) / (R A_fmt + U32 A_32)."""
    return {n: k_of(yard[n], ref[n].ref, unit_bound(ref[n], case.fmt), 1.0, allowance=ref[n].tiny) for n in ref}


def judge(case, ref, got, K):
    """Every element of every quantity of `ref` against its bound -> ({quantity: worst err / bound}, violations).  K: {quantity: K} or one
    number.  Where the bound is 0 (structural zeros) the element must be exactly zero; a NaN fails."""
    worst, bad = {}, []
    for n, qn in ref.items():
        b = bound(qn, case.fmt, K[n] if isinstance(K, dict) else K)
        g = got[n].double().reshape(qn.ref.shape)
        err = (g - qn.ref).abs()
        ok = err <= b
        ratio = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
        ratio = torch.nan_to_num(ratio, nan=float("inf"))
        worst[n] = float(ratio.max())
        if not bool(ok.all()):
            i = int(ratio.argmax())
            at = tuple(int(x) for x in torch.unravel_index(torch.tensor(i), qn.ref.shape))
            bad.append("%s %s: %d of %d elements outside the bound (%d of them structural zeros); the worst, at %s: got %r ref %r bound %.3e"
                       % (case.name(), n, int((~ok).sum()), ok.numel(), int((~ok & (b == 0)).sum()), at, float(g.reshape(-1)[i]),
                          float(qn.ref.reshape(-1)[i]), float(b.reshape(-1)[i])))
    return worst, bad


def old_check(got, ref, fmt, grad=False):
    """check() of tests/test_kernels_gpu.py at its own tolerance -> (accepted, figure)."""
    g, r = got.double(), ref.double().reshape(got.shape)
    if not bool(torch.isfinite(g).all()):
        return False, float("inf")
    err = float((g - r).abs().max() / (r.abs().max() + 1e-20))
    return err <= OLD_TOL[fmt] * (2 if grad else 1), err


def line(case, what, sel, ky, K, worst):
    cols = "  ".join("%s K_yard %5.3f K %5.2f worst %5.3f" % (n, ky[n], K[n], worst[n]) for n in worst)
    return "  %-42s %-9s %-8s k%s F%d b%d w%d | %s" % (case.name(), what, sel.family, "-" if sel.kch is None else sel.kch, sel.flags, sel.bits,
                                                       sel.waves, cols)


# ================================================================================================ token buffers, pads and guards
class Tokens:
    """[B, T, width] at token stride width + pad inside an allocation of token rows: GUARD rows, then per batch T rows and (unless dense)
    GUARD more; a dense one has GUARD rows after the last batch instead."""

    def __init__(self, B, T, width, dtype, dense=False):
        self.B, self.T, self.width, self.dtype = B, T, width, dtype
        self.es = 4 if dtype == torch.float32 else 2
        self.ld = width + (0 if dense else PAD)
        self.per = T + (0 if dense else GUARD)
        self.rows = GUARD + B * self.per + (GUARD if dense else 0)
        assert self.ld % 8 == 0 and (width * self.es) % 4 == 0

    def poison(self):
        idt = torch.int32 if self.es == 4 else torch.int16
        return torch.full((self.rows, self.ld), PATTERN if self.es == 4 else PATTERN & 0xFFFF, dtype=idt).view(self.dtype)

    def nan(self):
        return torch.full((self.rows, self.ld), float("nan"), dtype=self.dtype)

    def part(self, buf, t0, n, c0, w):
        """The [B, n, w] view of tokens t0 .. t0 + n, columns c0 .. c0 + w."""
        return buf[GUARD:GUARD + self.B * self.per].view(self.B, self.per, self.ld)[:, t0:t0 + n, c0:c0 + w]

    def put(self, buf, x, t0, c0):
        """x [B, H, n, hd] -> tokens t0.., columns c0 .. c0 + H hd."""
        B, H, n, hd = x.shape
        self.part(buf, t0, n, c0, H * hd).copy_(x.permute(0, 2, 1, 3).reshape(B, n, H * hd))

    def get(self, buf, t0, n, c0, H, hd):
        return self.part(buf, t0, n, c0, H * hd).reshape(self.B, n, H, hd).permute(0, 2, 1, 3).float()

    def offset(self, t0, c0):
        """Elements from the start of the allocation to (batch 0, token t0, column c0)."""
        return (GUARD + t0) * self.ld + c0

    def strides(self, hd):
        return (self.per * self.ld, self.ld, hd)

    def check(self, tag, buf, parts, bad):
        """buf: the whole allocation on the host after the call; parts: the (t0, n, c0, w) the call must have written, all of it."""
        idt = torch.int32 if self.es == 4 else torch.int16
        inside = torch.zeros(buf.shape, dtype=torch.bool)
        for p in parts:
            self.part(inside, *p).fill_(True)
        touched = (buf.view(idt) != self.poison().view(idt)) & ~inside
        if bool(touched.any()):
            r, col = [int(x[0]) for x in torch.nonzero(touched, as_tuple=True)]
            bad.append("%s: %d pad / guard words were written, the first at allocation row %d (batch %d token %d), column %d"
                       % (tag, int(touched.sum()), r, (r - GUARD) // self.per, (r - GUARD) % self.per, col))
        for p in parts:
            x = self.part(buf, *p).contiguous()
            if bool((x.view(torch.int32) == PATTERN).any()):
                bad.append("%s: %d logical 32-bit words still carry the pattern (never written)" % (tag, int((x.view(torch.int32) == PATTERN).sum())))
            if bool(torch.isnan(x.float()).any()):
                bad.append("%s: %d NaN" % (tag, int(torch.isnan(x.float()).sum())))


def flat_poison(n, dtype=torch.float32, guard=GUARD):
    """A flat output of n elements with `guard` elements of the pattern on either side (lse, delta, the bits, probs)."""
    if dtype == torch.uint8:
        return torch.full((n + 2 * guard,), PATTERN & 0xFF, dtype=torch.uint8)
    return torch.full((n + 2 * guard,), PATTERN, dtype=torch.int32).view(torch.float32)


def flat_check(tag, buf, n, bad, guard=GUARD, written=True):
    idt = torch.uint8 if buf.dtype == torch.uint8 else torch.int32
    pat = PATTERN & 0xFF if buf.dtype == torch.uint8 else PATTERN
    w = buf.view(idt)
    if bool((w[:guard] != pat).any()) or bool((w[guard + n:] != pat).any()):
        bad.append("%s: guard words were written" % tag)
    if written and buf.dtype != torch.uint8:
        if bool((w[guard:guard + n] == pat).any()):
            bad.append("%s: %d words still carry the pattern (never written)" % (tag, int((w[guard:guard + n] == pat).sum())))
        if bool(torch.isnan(buf[guard:guard + n]).any()):
            bad.append("%s: NaN" % tag)
