"""not gpu: the host side of IEEE-half encoder fine-tuning under a loss scale -- declaration / export / argument checks of
ecamp_sgd_scale_update, the opt-in `--fp16_loss_scale` flag on every command line of the reference's run_ft.sh, the opening line, and
`SGDLossScaler.host_update` against a table written out from apex's rule (LossScaler.update_scale, loss_scale="dynamic"):
overflow: scale x backoff, clean = 0, both skipped counters + 1; otherwise clean + 1, skipped-in-a-row = 0, and when clean == window
scale = min(max_scale, scale x growth), clean = 0; window 0: a static scale."""
import ctypes
import os

import pytest

from test_finetune_cpu import _run_ft_command_lines

ARGS = ["partials", "npart", "state", "ctl", "norm_out", "growth", "backoff", "window", "max_scale", "stream"]


def test_header_declares_the_scale_update_and_both_builds_export_and_check_it():
    from ecamp_amd import _lib
    if not all(os.path.exists(p) for p in _lib.LIB_PATHS.values()):
        from ecamp_amd import build
        build.build(verbose=False, half="both")
    protos = _lib.parse_header()
    assert _lib.abi_version_of_header() == 5          # an entry point was added, no signature changed
    assert "ecamp_sgd_scale_update" in protos and protos["ecamp_sgd_scale_update"][0] is ctypes.c_int32
    assert [n for _, n in protos["ecamp_sgd_scale_update"][1]] == ARGS and len(ARGS) == 10
    assert [t for t, _ in protos["ecamp_sgd_scale_update"][1]] == [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                                   ctypes.c_float, ctypes.c_float, ctypes.c_int32, ctypes.c_float, ctypes.c_void_p]
    one, null = ctypes.c_void_p(64), None
    for fmt in ("bf16", "f16"):
        lib = _lib.load(fmt)
        assert hasattr(lib, "ecamp_sgd_scale_update"), fmt
        err = lambda: lib.ecamp_last_error().decode()
        # argument errors are reported without a device: nothing is launched
        up = lambda part=one, npart=4, state=one, ctl=one, growth=2.0, backoff=0.5, window=2000, max_scale=2.0 ** 24: lib.ecamp_sgd_scale_update(
            part, npart, state, ctl, null, growth, backoff, window, max_scale, None)
        for kw in ({"part": null}, {"state": null}, {"ctl": null}):
            assert up(**kw) < 0 and "null pointer" in err(), kw
        assert up(npart=0) < 0 and "npart=0" in err()
        assert up(npart=4097) < 0 and "npart=4097" in err()
        assert up(npart=-1) < 0 and "npart=-1" in err()
        assert up(growth=0.5) < 0 and "growth=0.5" in err()
        assert up(backoff=0.0) < 0 and "backoff=0" in err()
        assert up(backoff=1.5) < 0 and "backoff=1.5" in err()
        assert up(window=-1) < 0 and "window=-1" in err()
        assert up(max_scale=0.0) < 0 and "max_scale=0" in err()
        assert up(max_scale=-4.0) < 0 and "max_scale=-4" in err()


# ---------------------------------------------------------------------------------------------------------------- driver
def _no_device(*a, **k):
    raise AssertionError("the flags must be checked before a model is built")


def test_every_command_line_of_run_ft_passes_with_only_the_loss_scale_flag_added(monkeypatch):
    from ecamp_amd import main_finetune
    monkeypatch.setattr(main_finetune, "build_model", _no_device)
    parse = main_finetune.get_args_parser().parse_args
    lines = _run_ft_command_lines()
    assert len(lines) == 12
    for argv, (task, C, vol, steps, eb, lr, wu, tb) in lines:
        assert "--fp16" in argv
        a = main_finetune.check_args(parse(argv + ["--fp16_loss_scale", "dynamic"]))
        assert a.compute_dtype == "fp16" and a.fp16_loss_scale == "dynamic" and a.mode == "Finetune"
        assert (a.task, a.num_classes, a.num_steps, a.learning_rate, a.train_batch_size) == (task, C, steps, lr, tb)
        a = main_finetune.check_args(parse(argv + ["--fp16_loss_scale", "1024"]))
        assert a.compute_dtype == "fp16" and main_finetune.loss_scale_of(a.fp16_loss_scale) == 1024.0
    # --compute_dtype fp16 in place of --fp16 selects the same mode; --loss_scale stays accepted and ignored
    argv = [x for x in lines[0][0] if x != "--fp16"] + ["--compute_dtype", "fp16", "--fp16_loss_scale", "dynamic", "--loss_scale", "128"]
    assert main_finetune.check_args(parse(argv)).compute_dtype == "fp16"
    assert parse(lines[0][0]).fp16_loss_scale is None       # the default: the mode is opt-in


@pytest.mark.parametrize("value", ["3", "0", "-8", "abc"])
def test_a_loss_scale_that_is_no_positive_power_of_two_is_refused_before_any_device_work(value, monkeypatch):
    from ecamp_amd import main_finetune
    monkeypatch.setattr(main_finetune, "build_model", _no_device)
    argv = _run_ft_command_lines()[0][0] + ["--fp16_loss_scale", value]
    with pytest.raises(SystemExit) as e:
        main_finetune.main(main_finetune.get_args_parser().parse_args(argv))
    assert e.value.code not in (0, None) and "--fp16_loss_scale %s" % value in str(e.value) and "power of two" in str(e.value)


@pytest.mark.parametrize("dtype", [["--compute_dtype", "bf16"], ["--compute_dtype", "fp32"], []], ids=["bf16", "fp32", "default"])
def test_the_loss_scale_flag_without_half_is_refused_before_any_device_work(dtype, monkeypatch):
    from ecamp_amd import main_finetune
    monkeypatch.setattr(main_finetune, "build_model", _no_device)
    argv = [x for x in _run_ft_command_lines()[0][0] if x != "--fp16"] + dtype + ["--fp16_loss_scale", "dynamic"]
    with pytest.raises(SystemExit) as e:
        main_finetune.main(main_finetune.get_args_parser().parse_args(argv))
    assert e.value.code not in (0, None) and "--fp16_loss_scale" in str(e.value) and "--compute_dtype fp16" in str(e.value)


def test_half_without_the_flag_is_still_refused_and_the_message_names_the_flag(monkeypatch):
    from ecamp_amd import main_finetune
    monkeypatch.setattr(main_finetune, "build_model", _no_device)
    with pytest.raises(SystemExit) as e:
        main_finetune.main(main_finetune.get_args_parser().parse_args(_run_ft_command_lines()[0][0]))
    for w in ("--fp16", "--compute_dtype bf16", "--fp16_loss_scale dynamic"):
        assert w in str(e.value), w


def test_the_probe_ignores_the_flag(monkeypatch):
    from ecamp_amd import main_finetune, main_linprobe
    seen = []
    monkeypatch.setattr(main_linprobe, "main", lambda args: seen.append(args) or "probe")
    monkeypatch.setattr(main_finetune, "build_model", _no_device)
    a = main_finetune.get_args_parser().parse_args(_run_ft_command_lines()[0][0] + ["--mode", "LinearProbe", "--fp16_loss_scale", "3"])
    assert main_finetune.main(a) == "probe" and seen == [a]
    b = main_linprobe.check_args(main_linprobe.get_args_parser().parse_args(
        [x for x in _run_ft_command_lines()[0][0] if x != "--fp16"] + ["--mode", "LinearProbe", "--fp16_loss_scale", "dynamic"]))
    assert b.compute_dtype == "bf16"


def test_opening_line_is_unchanged_at_defaults_and_says_what_the_half_mode_is():
    from ecamp_amd import main_finetune
    parse = main_finetune.get_args_parser().parse_args
    plain = [x for x in _run_ft_command_lines()[0][0] if x != "--fp16"]
    assert main_finetune.opening_line(main_finetune.check_args(parse(plain))) == main_finetune.DEVIATIONS
    assert main_finetune.opening_line(parse(plain)) == main_finetune.DEVIATIONS
    line = main_finetune.opening_line(main_finetune.check_args(parse(_run_ft_command_lines()[0][0] + ["--fp16_loss_scale", "dynamic"])))
    assert line.startswith(main_finetune.DEVIATIONS)
    for w in ("IEEE half", "f32 masters", "f32 head", "apex O2", "dynamic", "1048576", "2^20", "2000", "16777216", "skipped", "residual stream is half",
              "f32_residual"):
        assert w in line, w
    line = main_finetune.opening_line(main_finetune.check_args(parse(_run_ft_command_lines()[0][0] + ["--fp16_loss_scale", "4096", "--f32_residual"])))
    for w in ("static", "4096", "residual stream is f32", "--f32_residual"):
        assert w in line, w
    assert "dynamic" not in line


# ---------------------------------------------------------------------------------------------------------------- the rule
def _states(scaler, flags):
    out = []
    for f in flags:
        scaler.host_update(f)
        out.append((scaler.scale, scaler.clean_steps, scaler.skipped_steps, scaler.skipped_in_a_row))
    return out


def test_host_update_against_the_table_of_the_rule():
    from ecamp_amd.optim import SGDLossScaler
    s = SGDLossScaler()
    assert (s.scale, s.growth, s.backoff, s.window, s.max_scale) == (2.0 ** 20, 2.0, 0.5, 2000, 2.0 ** 24)
    assert (s.clean_steps, s.skipped_steps, s.skipped_in_a_row, s.last_found_inf) == (0, 0, 0, False)
    # window 3 from 8, at most 32: (found) -> (scale, clean, skipped, skipped in a row)
    table = [(0, (8, 1, 0, 0)), (0, (8, 2, 0, 0)), (0, (16, 0, 0, 0)),      # growth exactly at the window, the clean count starts again
             (1, (8, 0, 1, 1)), (1, (4, 0, 2, 2)),                           # backoff; both skipped counters
             (0, (4, 1, 2, 0)),                                              # a clean step ends the run of skips, the total stays
             (0, (4, 2, 2, 0)), (1, (2, 0, 3, 1)),                           # an overflow one step short of the window resets the clean count
             (0, (2, 1, 3, 0)), (0, (2, 2, 3, 0)), (0, (4, 0, 3, 0)),
             (0, (4, 1, 3, 0)), (0, (4, 2, 3, 0)), (0, (8, 0, 3, 0)),
             (0, (8, 1, 3, 0)), (0, (8, 2, 3, 0)), (0, (16, 0, 3, 0)),
             (0, (16, 1, 3, 0)), (0, (16, 2, 3, 0)), (0, (32, 0, 3, 0)),
             (0, (32, 1, 3, 0)), (0, (32, 2, 3, 0)), (0, (32, 0, 3, 0))]     # the cap: min(max_scale, 64)
    s = SGDLossScaler(init_scale=8, window=3, max_scale=32)
    got = _states(s, [f for f, _ in table])
    assert got == [tuple(map(float, w[:1])) + w[1:] for _, w in table]
    assert s.last_found_inf is False and s.host_update(True) == 16.0 and s.last_found_inf is True
    # window 0: the scale never moves, an overflow still counts as a skipped step
    s = SGDLossScaler(init_scale=1024, window=0)
    got = _states(s, [0, 0, 1, 1, 0, 0, 0])
    assert [g[0] for g in got] == [1024.0] * 7 and got[3] == (1024.0, 0, 2, 2) and got[-1] == (1024.0, 3, 2, 0)
    # no floor: 21 halvings from 2^20 reach 0.5
    s = SGDLossScaler()
    assert _states(s, [1] * 21)[-1] == (0.5, 0, 21, 21)
    for bad in (dict(init_scale=0), dict(growth=0.5), dict(backoff=0), dict(backoff=1.5), dict(window=-1), dict(max_scale=0)):
        with pytest.raises(ValueError):
            SGDLossScaler(**bad)
