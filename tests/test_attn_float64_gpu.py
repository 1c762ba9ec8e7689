"""-m gpu: the attention kernels behind ecamp_attn_fwd / ecamp_attn_bwd / ecamp_attn_probs -- the head-resident kernels, the resident
forward, the 64-row streaming backward pair and the long forward of csrc/attention_bf16.hip, the f32 kernels of csrc/attention.hip with
their one-wave-per-row form -- held to float64 element by element.  Reference, magnitudes, yardstick, bounds, regimes, case tables,
buffers and the restated kernel selection are those of tests/_attn_ref.py (read its docstring first); tests/test_attn_reference_cpu.py
proves them without a GPU.

Every case is one forward call and one backward call on the O and lse that forward call stored -- two backward calls where the forward
left dropout bits: one reading them, one regenerating the mask.  Every call
  * goes through hip_ops.call on buffers the test owns, in the production layouts of ecamp_amd/functions.py (packed qkv, or q dense with
    k / v from token 1 of a [B, Tk + 1, 2D] buffer): token stride width + 8, 8 guard token rows before the first batch and after every
    batch; input pads, guards, rows that are not the operand's and the cross buffer's token 0 hold NaN; O, lse, dQ, dK, dV, delta and the
    bits are pre-filled with 0x5A5A5A5A with guards.  Afterwards every pad and guard word is intact (the cross buffer's token-0 row of
    dK / dV too), no logical word carries the pattern and nothing is NaN.  One dense call per family keeps the wrap-around layout;
  * proves what ran twice: by the profiler tag attn:<family>:<f|b>:<hd>:<Tq>:<Tk>:k<kch>F<FLAGS>b<bits>w<waves>, which must be the one of
    the table written by hand in _attn_ref.GPU_CASES / F32_CASES (and of the mirror _attn_ref.select), and by ecamp_attn_head_launches
    moving by one for a head-resident launch and not at all otherwise;
  * is judged in EVERY element of O, lse, dQ, dK and dV; where the magnitude is zero (rows of keys behind the mask) the element must be
    zero; prints K_yard, K and its worst err / bound per quantity (profiles/attn_float64.txt is one run's output).

Out of scope: fully masked batches, head widths other than 32 / 64 / 128, the ECAMP_ATTN_WAVES override, subnormal operands."""
import ctypes

import pytest
import torch

import _attn_ref as A
from _attn_ref import BF16, DTYPE, F16, F32, Case, Tokens

pytestmark = pytest.mark.gpu


def _ops():
    from ecamp_amd import hip_ops
    return hip_ops


def _lib():
    from ecamp_amd import _lib as L
    return L.load()


def _fmt():
    from ecamp_amd import _lib as L
    return F16 if L.half() == "f16" else BF16


@pytest.fixture
def head_switch():
    """set(v): set_option("attn_head", v); back to the environment's choice afterwards."""
    o = _ops()
    try:
        yield lambda v: o.set_option("attn_head", v)
    finally:
        o.set_option("attn_head", -1)


def _tags():
    lib = _lib()
    n = int(lib.ecamp_prof_dump(None, 0))
    buf = ctypes.create_string_buffer(n + 16)
    lib.ecamp_prof_dump(buf, len(buf))
    return [ln.split()[0] for ln in buf.value.decode().splitlines() if ln.startswith("attn:")]


class _Dev:
    """A Tokens allocation on the device with the places of the operands inside it."""

    def __init__(self, dev, tok, host):
        self.tok, self.t = tok, host.to(dev)

    def ptr(self, t0=0, c0=0):
        return ctypes.c_void_p(self.t.data_ptr() + self.tok.offset(t0, c0) * self.tok.es)

    def host(self):
        return self.t.cpu()


def _flat_ptr(t, guard=A.GUARD):
    return ctypes.c_void_p(t.data_ptr() + guard * t.element_size())


def _profiled(fn):
    """fn() between a clear and a dump of the profiler -> (the attention tags it left, head-resident launches it made)."""
    lib = _lib()
    h0 = int(lib.ecamp_attn_head_launches())
    lib.ecamp_prof_collect(-1, None, None, None)
    lib.ecamp_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        lib.ecamp_prof_enable(0)
    tags = _tags()
    lib.ecamp_prof_collect(-1, None, None, None)
    return tags, int(lib.ecamp_attn_head_launches()) - h0


def _prove(c, what, tags, moved, want, mirror, backward):
    assert want == mirror, "%s %s: the hand-written table says %s, the restated selection %s" % (c.name(), what, want, mirror)
    assert tags == [A.tag_of(want, backward, c.hd, c.Tq, c.Tk)], (c.name(), what, tags, want)
    assert moved == int(want.family == "head"), "%s %s: ecamp_attn_head_launches moved by %d, %s expected" % (c.name(), what, moved, want)


def run_case(dev, fmt, case_id, regime, dense=False):
    """The forward call and the backward call(s) of one case: launches, proves what ran, checks every pad and guard, judges every element."""
    o, lib = _ops(), _lib()
    layout, (B, H, Tq, Tk, hd), masked, p, head, want_f, want_bb, want_br = A.intended(case_id)
    c = Case(fmt, B, H, Tq, Tk, hd, regime, masked, p)
    dt, D, code = DTYPE[fmt], H * hd, o.code(DTYPE[fmt])
    keep = o.dropout_mask((B, H, Tq, Tk), dev, p, A.SEED, A.OFFSET).float().cpu() if p > 0 else c.ones()
    assert p == 0 or abs(float(keep.mean()) - (1 - p)) < 0.03
    km = c.key_mask.to(dev) if masked else None

    # ---- the operands in their layout: (allocation, first token, first column) of q, k, v; the gradients mirror them
    if layout == "packed":
        tok = Tokens(B, max(Tq, Tk), 3 * D, dt, dense)
        place = {"q": (tok, 0, 0), "k": (tok, 0, D), "v": (tok, 0, 2 * D)}
        hosts = {id(tok): tok.nan()}
    else:
        tq, tkv = Tokens(B, Tq, D, dt, dense), Tokens(B, Tk + 1, 2 * D, dt, dense)
        place = {"q": (tq, 0, 0), "k": (tkv, 1, 0), "v": (tkv, 1, D)}
        hosts = {id(tq): tq.nan(), id(tkv): tkv.nan()}
    for n, x in (("q", c.q), ("k", c.k), ("v", c.v)):
        t, t0, c0 = place[n]
        t.put(hosts[id(t)], x, t0, c0)
    ins = {i: _Dev(dev, t, hosts[i]) for i, t in {id(place[n][0]): place[n][0] for n in place}.items()}
    arg = lambda n: ins[id(place[n][0])].ptr(place[n][1], place[n][2])       # noqa: E731
    st = lambda n: o._st(place[n][0].strides(hd))                            # noqa: E731
    len_of = {"q": Tq, "k": Tk, "v": Tk}
    to, tdo = Tokens(B, Tq, D, dt, dense), Tokens(B, Tq, D, dt, dense)
    hdo = tdo.nan()
    tdo.put(hdo, c.do, 0, 0)
    dO = _Dev(dev, tdo, hdo)
    nb = int(lib.ecamp_attn_mask_bytes(B, H, Tq, Tk, hd, code))
    assert nb == A.mask_bytes(B, H, Tq, Tk, hd, fmt, head)
    has_bits = p > 0 and nb > 0
    assert has_bits == (want_bb is not None)
    bad = []

    # ---- forward
    O = _Dev(dev, to, to.poison())
    lse = A.flat_poison(B * H * Tq).to(dev)
    bits = A.flat_poison(nb, torch.uint8, 32).to(dev) if has_bits else None
    tags, moved = _profiled(lambda: o.call(
        "ecamp_attn_fwd", arg("q"), arg("k"), arg("v"), O.ptr(), _flat_ptr(lse), o.ptr(km), B, H, Tq, Tk, hd, st("q"), st("k"), st("v"),
        o._st(to.strides(hd)), c.scale, float(p), A.SEED, A.OFFSET, code, _flat_ptr(bits, 32) if has_bits else ctypes.c_void_p(0), o.stream()))
    _prove(c, "forward", tags, moved, want_f, A.select(fmt, Tq, Tk, hd, masked or p > 0, has_bits, False, head), False)
    hO, hlse = O.host(), lse.cpu()
    to.check("%s O" % c.name(), hO, [(0, Tq, 0, D)], bad)
    A.flat_check("%s lse" % c.name(), hlse, B * H * Tq, bad)
    if has_bits:
        A.flat_check("%s bits" % c.name(), bits.cpu(), nb, bad, guard=32)
    assert not bad, bad
    got = {"O": to.get(hO, 0, Tq, 0, H, hd), "lse": hlse[A.GUARD:A.GUARD + B * H * Tq].reshape(B, H, Tq)}
    ref = c.forward(keep)
    ky = A.k_yard_of(c, ref, c.fwd_outputs(keep, yard=True))
    K = {n: A.bound_k(v) for n, v in ky.items()}
    worst, bad = A.judge(c, ref, got, K)
    print(A.line(c, "forward" + (" dense" if dense else ""), want_f, ky, K, worst))
    assert not bad, bad

    # ---- backward, on the O and lse this forward call stored
    refb = c.backward(got["O"], got["lse"], keep)
    kyb = A.k_yard_of(c, refb, c.bwd_outputs(got["O"], got["lse"], keep, yard=True))
    Kb = {n: A.bound_k(v) for n, v in kyb.items()}
    lse_in = torch.full_like(hlse, float("nan"))
    lse_in[A.GUARD:A.GUARD + B * H * Tq] = hlse[A.GUARD:A.GUARD + B * H * Tq]
    lse_in = lse_in.to(dev)
    hO_in = to.nan()
    to.part(hO_in, 0, Tq, 0, D).copy_(to.part(hO, 0, Tq, 0, D))
    O_in = _Dev(dev, to, hO_in)
    gname = {"q": "dQ", "k": "dK", "v": "dV"}
    results = []
    for use_bits, want in ((True, want_bb), (False, want_br)):
        if want is None:
            continue
        gh = {i: _Dev(dev, ins[i].tok, ins[i].tok.poison()) for i in ins}
        garg = lambda n: gh[id(place[n][0])].ptr(place[n][1], place[n][2])   # noqa: E731
        delta = A.flat_poison(B * H * Tq).to(dev)
        assert int(lib.ecamp_attn_bwd_workspace_bytes(B, H, Tq)) == B * H * Tq * 4
        tags, moved = _profiled(lambda: o.call(
            "ecamp_attn_bwd", arg("q"), arg("k"), arg("v"), O_in.ptr(), dO.ptr(), _flat_ptr(lse_in), _flat_ptr(delta), garg("q"), garg("k"), garg("v"),
            o.ptr(km), B, H, Tq, Tk, hd, st("q"), st("k"), st("v"), o._st(to.strides(hd)), o._st(tdo.strides(hd)), st("q"), st("k"), st("v"),
            c.scale, float(p), A.SEED, A.OFFSET, code, _flat_ptr(bits, 32) if use_bits else ctypes.c_void_p(0), o.stream()))
        what = "backward " + ("bits" if use_bits else "regen" if p > 0 else "")
        _prove(c, what, tags, moved, want, A.select(fmt, Tq, Tk, hd, masked or p > 0, use_bits, True, head), True)
        gotb = {}
        for i, g in gh.items():
            h = g.host()
            parts = [(place[n][1], len_of[n], place[n][2], D) for n in place if id(place[n][0]) == i]
            g.tok.check("%s %s gradients" % (c.name(), what), h, parts, bad)
            for n in place:
                if id(place[n][0]) == i:
                    gotb[gname[n]] = g.tok.get(h, place[n][1], len_of[n], place[n][2], H, hd)
        A.flat_check("%s %s delta" % (c.name(), what), delta.cpu(), B * H * Tq, bad)
        assert not bad, bad
        worst, bad = A.judge(c, refb, gotb, Kb)
        print(A.line(c, what + (" dense" if dense else ""), want, kyb, Kb, worst))
        assert not bad, bad
        results.append(gotb)
    if len(results) == 2:      # the saved bits ARE the regenerated mask
        for n in results[0]:
            assert torch.equal(results[0][n], results[1][n]), "%s %s: saved bits and regenerated mask disagree" % (c.name(), n)
    for i in ins:              # no input was written
        if True:
            assert torch.equal(ins[i].host().view(torch.int16), hosts[i].view(torch.int16))


_HALF_RUNS, _F32_RUNS = A.gpu_runs()


@pytest.mark.parametrize("case_id,regime", _HALF_RUNS)
def test_attention_16bit(dev, both_halves, head_switch, case_id, regime):
    """Both 16-bit builds: every family of attn16_select at the smallest shapes that reach each of its paths (the table and the reason
    for every shape: _attn_ref.GPU_CASES)."""
    head_switch(A.intended(case_id)[4])
    run_case(dev, _fmt(), case_id, regime)
    if regime == "plain" and case_id in A.DENSE:
        run_case(dev, _fmt(), case_id, regime, dense=True)


@pytest.mark.parametrize("case_id,regime", _F32_RUNS)
def test_attention_f32(dev, head_switch, case_id, regime):
    """f32 operands: the exact-f32 MFMA kernels at 1, 2 and 4 key chunks and the one-wave-per-row kernels past 256 keys."""
    head_switch(A.intended(case_id)[4])
    run_case(dev, F32, case_id, regime)
    if regime == "plain" and case_id in A.DENSE:
        run_case(dev, F32, case_id, regime, dense=True)


def _probs(dev, fmt, case_id):
    o = _ops()
    (B, H, Tq, Tk, hd), masked = A.PROBS_CASES[case_id]
    c = Case(fmt, B, H, Tq, Tk, hd, "plain", masked)
    dt, D = DTYPE[fmt], H * hd
    tq, tkv = Tokens(B, Tq, D, dt), Tokens(B, Tk + 1, 2 * D, dt)
    hq, hkv = tq.nan(), tkv.nan()
    tq.put(hq, c.q, 0, 0)
    tkv.put(hkv, c.k, 1, 0)
    Q, KV = _Dev(dev, tq, hq), _Dev(dev, tkv, hkv)
    n = B * H * Tq * Tk
    probs = A.flat_poison(n).to(dev)
    km = c.key_mask.to(dev) if masked else None
    o.call("ecamp_attn_probs", Q.ptr(), KV.ptr(1, 0), o.ptr(km), _flat_ptr(probs), B, H, Tq, Tk, hd, o._st(tq.strides(hd)), o._st(tkv.strides(hd)),
           c.scale, o.code(dt), o.stream())
    torch.cuda.synchronize()
    bad, h = [], probs.cpu()
    A.flat_check("%s probs" % c.name(), h, n, bad)
    assert not bad, bad
    ref = c.probs()
    ky = A.k_yard_of(c, ref, c.probs_yard())
    K = {k: A.bound_k(v) for k, v in ky.items()}
    worst, bad = A.judge(c, ref, {"probs": h[A.GUARD:A.GUARD + n].reshape(B, H, Tq, Tk)}, K)
    print("  %-42s probs     K_yard %5.3f K %5.2f worst %5.3f" % (c.name(), ky["probs"], K["probs"], worst["probs"]))
    assert not bad, bad


@pytest.mark.parametrize("case_id", sorted(A.PROBS_CASES))
def test_attention_probs_16bit(dev, both_halves, case_id):
    """ecamp_attn_probs (one wave per query row, f32 output): q dense, k from token 1 of a [B, Tk + 1, 2D] buffer; judged against the
    float64 P with the f32 part of the bound, exactly zero behind the mask."""
    _probs(dev, _fmt(), case_id)


@pytest.mark.parametrize("case_id", sorted(A.PROBS_CASES))
def test_attention_probs_f32(dev, case_id):
    _probs(dev, F32, case_id)
