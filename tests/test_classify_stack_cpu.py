"""not gpu: the host side that the classification stack shares -- the checkpoint packing of optim._FlatOptimizer (FusedAdamW and FusedSGD
over arena.FlatSpace stand-ins in host memory) and the split of the drivers' `check_args` into their own refusals and one shared remainder."""
import pytest
import torch

from ecamp_amd import arena, hip_ops, main_finetune, main_linprobe, optim

SIZES = [1, 63, 64, 65, 130, 4096]
UNUSED = 2


class _HostSpace(arena.FlatSpace):
    """A FlatSpace in host memory with what the optimizers ask of an arena (tail=False) or of a FlatTail (tail=True)."""

    def __init__(self, named, tail=False):
        super().__init__(list(named), torch.device("cpu"))
        self.flat_p16, self.reducer, self.version = None, None, 0
        if tail:
            self.flat_buf = torch.zeros(self.total)
        for p in self.params:
            setattr(p, "_ecamp_tail" if tail else "_ecamp_arena", self)

    def zero_grad(self):
        self.flat_g.zero_()

    def flush_fresh(self):
        pass


@pytest.fixture
def spaces(monkeypatch):
    monkeypatch.setattr(hip_ops, "zeros", lambda shape, dev: torch.zeros(shape, dtype=torch.float32, device=dev))
    monkeypatch.setattr(hip_ops, "sumsq_grouped_slots", lambda n: 1)
    g = torch.Generator().manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(n, generator=g)) for n in SIZES[:-1]] + [torch.nn.Parameter(torch.randn(64, 64, generator=g))]
    ps[UNUSED]._ecamp_unused = True
    tl = [torch.nn.Parameter(torch.randn(192, generator=g)), torch.nn.Parameter(torch.randn(3, 192, generator=g))]
    return ps, tl, _HostSpace([("p%d" % i, p) for i, p in enumerate(ps)]), _HostSpace([("t0", tl[0]), ("t1", tl[1])], tail=True), g


def _groups(ps):
    return [{"params": ps[:3], "weight_decay": 0.0}, {"params": ps[3:], "weight_decay": 0.05}]


def test_adamw_state_dict_is_torch_adamw_layout_entry_for_entry(spaces):
    ps, _, A, _, g = spaces
    opt = optim.FusedAdamW(_groups(ps), lr=1e-3, betas=(0.9, 0.95))
    sd = opt.state_dict()
    assert sd["state"] == {} and [grp["params"] for grp in sd["param_groups"]] == [[0, 1, 2], [3, 4, 5]]
    assert opt._table.tolist() == [0, 0, 255, 1, 1] + [1] * 67 and opt._tail is None
    opt._m.copy_(torch.randn(A.total, generator=g))
    opt._v.copy_(torch.rand(A.total, generator=g))
    opt._step = 7
    sd = opt.state_dict()
    assert list(sd["state"]) == [0, 1, 3, 4, 5]                       # the unused parameter has no state, as torch skips `grad is None`
    assert list(sd["param_groups"][0]) == ["weight_decay", "lr", "betas", "eps", "params"]   # the group's own order, `params` last
    for i, e in sd["state"].items():
        o, n = A.span(ps[i])
        assert list(e) == ["step", "exp_avg", "exp_avg_sq"] and float(e["step"]) == 7.0
        assert torch.equal(e["exp_avg"], opt._m[o:o + n].view(ps[i].shape)) and torch.equal(e["exp_avg_sq"], opt._v[o:o + n].view(ps[i].shape))
        assert e["exp_avg"].data_ptr() != opt._m[o:o + n].data_ptr()  # a copy, not a view
    ref = torch.optim.AdamW(_groups([torch.nn.Parameter(p.detach().clone()) for p in ps]), lr=1e-3, betas=(0.9, 0.95))
    ref.load_state_dict(sd)                                           # torch accepts it
    for keys in (int, str):
        twin = optim.FusedAdamW(_groups(ps), lr=5e-3, betas=(0.9, 0.95))
        twin.load_state_dict({"state": {keys(k): v for k, v in sd["state"].items()}, "param_groups": sd["param_groups"]})
        assert twin._step == 7 and twin.param_groups[0]["lr"] == 1e-3
        back = twin.state_dict()
        assert list(back["state"]) == list(sd["state"])
        assert all(torch.equal(back["state"][i][k], sd["state"][i][k]) for i in sd["state"] for k in ("step", "exp_avg", "exp_avg_sq"))


def test_sgd_state_dict_covers_arena_and_tail_and_skips_empty_buffers(spaces):
    ps, tl, A, T, g = spaces
    opt = optim.FusedSGD(ps + tl, lr=3e-2, momentum=0.9, weight_decay=1e-4, max_grad_norm=1.0)
    assert opt.state_dict()["state"] == {}
    assert opt._table.tolist() == [0, 0, 255] + [0] * 69 and opt._tail_table.tolist() == [0] * (T.total // 64) and opt._tail is T
    opt._buf.copy_(torch.randn(A.total, generator=g))
    T.flat_buf.copy_(torch.randn(T.total, generator=g))
    opt._steps = 3
    sd = opt.state_dict()
    assert list(sd["state"]) == [0, 1, 3, 4, 5, 6, 7]
    assert list(sd["param_groups"][0]) == ["lr", "momentum", "dampening", "weight_decay", "nesterov", "params"]
    for i, e in sd["state"].items():
        p = (ps + tl)[i]
        space, buf = (A, opt._buf) if i < len(ps) else (T, T.flat_buf)
        o, n = space.span(p)
        assert list(e) == ["momentum_buffer"] and torch.equal(e["momentum_buffer"], buf[o:o + n].view(p.shape))
    want_arena, want_tail = torch.zeros(A.total), torch.zeros(T.total)   # what a load restores: the saved spans, not padding, not entry 1
    for i in (0, 3, 4, 5):
        o, n = A.span(ps[i])
        want_arena[o:o + n] = opt._buf[o:o + n]
    for p in tl:
        o, n = T.span(p)
        want_tail[o:o + n] = T.flat_buf[o:o + n]
    opt._buf.zero_()
    T.flat_buf.zero_()
    state = {str(k): v for k, v in sd["state"].items()}
    state["1"] = {"momentum_buffer": None}                            # torch.optim.SGD before its first step: nothing to load
    twin = optim.FusedSGD(ps + tl, lr=1e-2, momentum=0.9)
    twin.load_state_dict({"state": state, "param_groups": sd["param_groups"]})
    assert twin._steps == 1 and twin.param_groups[0]["lr"] == 3e-2
    assert torch.equal(twin._buf, want_arena) and torch.equal(T.flat_buf, want_tail)


def test_binding_errors_name_the_class(spaces):
    ps, tl, _, _, g = spaces
    loose = torch.nn.Parameter(torch.zeros(4))
    for cls in (optim.FusedAdamW, optim.FusedSGD):
        with pytest.raises(RuntimeError, match="^%s: parameter is not in an ecamp_amd arena -- call model.prepare" % cls.__name__):
            cls([loose]).arena
        other = _HostSpace([("q", torch.nn.Parameter(torch.zeros(5)))])
        with pytest.raises(RuntimeError, match="^%s: parameters from different arenas$" % cls.__name__):
            cls([ps[0], other.params[0]]).arena
        with pytest.raises(ValueError, match="^%s supports at most 8 param groups$" % cls.__name__):
            cls([{"params": [torch.nn.Parameter(torch.zeros(2))]} for _ in range(9)])
    with pytest.raises(RuntimeError, match="not in an ecamp_amd arena"):   # a tail parameter means nothing to AdamW
        optim.FusedAdamW(tl).arena
    with pytest.raises(RuntimeError, match=r"^FusedSGD: no parameter of a model's arena among the groups \(the tail buffer alone is not supported\)$"):
        optim.FusedSGD(tl).arena
    tail2 = _HostSpace([("u", torch.nn.Parameter(torch.zeros(5)))], tail=True)
    with pytest.raises(RuntimeError, match=r"^FusedSGD: parameters from different arenas \(two tail buffers\)$"):
        optim.FusedSGD([ps[0], tl[0], tail2.params[0]]).arena


# ---------------------------------------------------------------------------------------------------------------- check_args
def _parse(*argv):
    return main_linprobe.get_args_parser().parse_args(["--name", "t", *argv])


def test_each_driver_refuses_the_others_mode_and_its_own_cases_first():
    with pytest.raises(SystemExit, match="--mode Finetune is not implemented here: this driver trains the linear probe only"):
        main_linprobe.check_args(_parse("--synthetic", "--local_rank", "0"))
    with pytest.raises(SystemExit, match="data-parallel probing is not implemented here"):
        main_linprobe.check_args(_parse("--synthetic", "--mode", "LinearProbe", "--local_rank", "0", "--num_classes", "65"))
    with pytest.raises(SystemExit, match="^--gradient_accumulation_steps other than 1 is not implemented here$"):
        main_linprobe.check_args(_parse("--synthetic", "--mode", "LinearProbe", "--gradient_accumulation_steps", "2"))
    with pytest.raises(SystemExit, match="this driver fine-tunes the encoder"):
        main_finetune.check_args(_parse("--synthetic", "--mode", "Other"))
    with pytest.raises(SystemExit, match="data-parallel fine-tuning is not implemented here"):
        main_finetune.check_args(_parse("--synthetic", "--local_rank", "0", "--num_classes", "65"))
    with pytest.raises(SystemExit, match="^--gradient_accumulation_steps 2: gradient accumulation is not implemented here"):
        main_finetune.check_args(_parse("--synthetic", "--gradient_accumulation_steps", "2"))
    with pytest.raises(SystemExit, match="--fp16 --mode Finetune is not implemented here"):
        main_finetune.check_args(_parse("--synthetic", "--compute_dtype", "fp16"))


@pytest.mark.parametrize("flags, text", [
    (["--synthetic", "--num_classes", "65"], r"^--num_classes must lie in \[1, 64\]$"),
    ([], r"^--stage train needs --pretrained_path"),
    (["--pretrained_path", "x.pth"], r"^--dataset_path is required \(or --synthetic\)$")])
def test_the_shared_remainder_refuses_alike_and_leaves_the_mode_alone(flags, text):
    for mod, mode in ((main_linprobe, "LinearProbe"), (main_finetune, "Finetune")):
        args = _parse("--mode", mode, *flags)
        with pytest.raises(SystemExit, match=text):
            mod.check_args(args)
        assert args.mode == mode
    with pytest.raises(SystemExit, match="--fp16 contradicts --compute_dtype bf16"):
        main_linprobe.check_args(_parse("--mode", "LinearProbe", "--synthetic", "--fp16", "--compute_dtype", "bf16"))


def test_accepted_arguments_get_the_same_defaults_from_both_drivers():
    flags = ["--synthetic", "--task", "COVIDx", "--stage", "test"]
    a = main_linprobe.check_args(_parse("--mode", "LinearProbe", *flags))
    b = main_finetune.check_args(_parse(*flags))
    assert (a.mode, b.mode) == ("LinearProbe", "Finetune")
    va, vb = dict(vars(a), mode=None), dict(vars(b), mode=None)
    assert va == vb and a.compute_dtype == "bf16" and a.is_multilabel is False and a.list_dir.replace("\\", "/") == "datasets/COVIDx"
    c = main_linprobe.check_common(_parse("--mode", "Other", "--synthetic", "--fp16", "--list_dir", "L"))   # the remainder does not read --mode
    assert c.compute_dtype == "fp16" and c.is_multilabel is True and c.list_dir == "L" and c.mode == "Other"
