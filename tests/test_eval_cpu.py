"""not gpu: the host side of held-out evaluation -- the driver's flags, the aggregation of an evaluation pass's sums
(engine_pretrain.eval_batch_sums / eval_stats) and the declaration / export of `ecamp_ce_eval`."""
import argparse
import ctypes
import os

import pytest
import torch


def _parse(argv):
    from ecamp_amd.main_pretrain import get_args_parser
    return argparse.ArgumentParser(parents=[get_args_parser()]).parse_args(argv)


def test_parser_defaults_leave_evaluation_off():
    a = _parse([])
    assert a.eval_freq == 0 and a.eval_only is False and a.val_data_path == "" and a.val_batch_size is None


@pytest.mark.parametrize("argv", [["--eval_freq", "1"], ["--eval_only", "--resume", "x.pth"], ["--eval_only", "--synthetic"]])
def test_evaluation_flags_are_checked_before_any_device_work(argv, monkeypatch):
    from ecamp_amd import main_pretrain
    from ecamp_amd.util import misc

    def no_device(*a, **k):
        raise AssertionError("the flags must be refused before the process group / the device is touched")

    monkeypatch.setattr(misc, "init_distributed_mode", no_device)
    with pytest.raises(SystemExit) as e:
        main_pretrain.main(_parse(["--lr", "1e-3"] + argv))
    assert "--val_data_path" in str(e.value) or "--resume" in str(e.value)


def test_evaluation_flags_accepted():
    from ecamp_amd.main_pretrain import check_eval_args
    check_eval_args(_parse([]))
    check_eval_args(_parse(["--eval_freq", "2", "--synthetic"]))
    check_eval_args(_parse(["--eval_freq", "2", "--val_data_path", "/data/held_out"]))
    check_eval_args(_parse(["--eval_only", "--resume", "c.pth", "--val_data_path", "/data/held_out"]))


def _sums(losses, counts, n):
    from ecamp_amd.engine_pretrain import eval_batch_sums
    return eval_batch_sums(torch.tensor(losses, dtype=torch.float32), torch.tensor(counts, dtype=torch.int64), n)


def test_aggregation_weights_a_short_last_batch_by_its_size_and_pools_the_counts():
    from ecamp_amd.engine_pretrain import EVAL_KEYS, eval_stats
    # two full batches of 4 and a last one of 2
    total = _sums([1.0, 2.0, 8.0], [10, 5, 8], 4) + _sums([3.0, 4.0, 6.0], [30, 3, 12], 4) + _sums([5.0, 0.5, 1.0], [0, 0, 0], 2)
    assert total.dtype == torch.float64 and total.shape == (7,)
    st = eval_stats(total.tolist())
    assert tuple(st) == EVAL_KEYS
    assert st["val_mim_loss"] == pytest.approx((4 * 1.0 + 4 * 3.0 + 2 * 5.0) / 10, rel=1e-12)
    assert st["val_res_loss"] == pytest.approx((4 * 2.0 + 4 * 4.0 + 2 * 0.5) / 10, rel=1e-12)
    assert st["val_mlm_loss"] == pytest.approx((4 * 8.0 + 4 * 6.0 + 2 * 1.0) / 10, rel=1e-12)
    # pooled: 8 / 40 and 20 / 40 -- the mean of the per-batch ratios (0.5, 0.1, undefined) would be something else
    assert st["val_mlm_top1"] == 8 / 40 and st["val_mlm_top5"] == 20 / 40
    assert st["val_mlm_tokens"] == 40 and isinstance(st["val_mlm_tokens"], int)


def test_aggregation_without_a_scored_token_reports_zero_not_nan():
    from ecamp_amd.engine_pretrain import eval_stats
    st = eval_stats((_sums([1.5, 2.5, 0.0], [0, 0, 0], 3) + _sums([0.5, 0.5, 0.0], [0, 0, 0], 1)).tolist())
    assert st["val_mlm_tokens"] == 0 and st["val_mlm_top1"] == 0.0 and st["val_mlm_top5"] == 0.0
    assert st["val_mim_loss"] == pytest.approx((3 * 1.5 + 0.5) / 4) and st["val_mlm_loss"] == 0.0
    empty = eval_stats([0.0] * 7)   # an empty loader
    assert all(v == 0 for v in empty.values())


def test_aggregation_over_two_ranks_is_the_sum_of_their_sums():
    """What the pass's one all-reduce does: the ranks' 7-vectors are added; the result is what one rank over all batches would report."""
    from ecamp_amd.engine_pretrain import eval_stats
    batches = [([1.0, 2.0, 3.0], [7, 3, 5], 4), ([2.0, 1.0, 4.0], [9, 1, 6], 4), ([4.0, 4.0, 2.0], [5, 5, 5], 4), ([8.0, 0.0, 1.0], [2, 0, 1], 1)]
    rank0 = sum(_sums(*b) for b in batches[0::2])
    rank1 = sum(_sums(*b) for b in batches[1::2])
    one = sum(_sums(*b) for b in batches)
    assert eval_stats((rank0 + rank1).tolist()) == eval_stats(one.tolist())
    st = eval_stats((rank0 + rank1).tolist())
    assert st["val_mlm_tokens"] == 23 and st["val_mlm_top1"] == 9 / 23 and st["val_mlm_top5"] == 17 / 23
    assert st["val_mim_loss"] == pytest.approx((4 * 1 + 4 * 2 + 4 * 4 + 8) / 13, rel=1e-12)
    # counts stay exact far beyond f32's 2^24
    big = eval_stats((_sums([0, 0, 0], [2 ** 40 + 1, 2 ** 40, 2 ** 40], 1) + _sums([0, 0, 0], [1, 1, 1], 1)).tolist())
    assert big["val_mlm_tokens"] == 2 ** 40 + 2


def test_noise_keys_are_fixed_and_distinct_per_rank_and_batch():
    from ecamp_amd.engine_pretrain import eval_noise_key
    keys = {eval_noise_key(r, i) for r in range(8) for i in range(100)}
    assert len(keys) == 800 and len({k[0] for k in keys}) == 1
    assert eval_noise_key(3, 17) == eval_noise_key(3, 17)
    assert all(0 <= off < 2 ** 64 for _, off in keys)


def test_header_declares_ce_eval_and_both_builds_export_it():
    from ecamp_amd import _lib
    if not all(os.path.exists(p) for p in _lib.LIB_PATHS.values()):
        from ecamp_amd import build
        build.build(verbose=False, half="both")
    protos = _lib.parse_header()
    assert "ecamp_ce_eval" in protos
    ret, args = protos["ecamp_ce_eval"]
    assert ret is ctypes.c_int32
    assert [n for _, n in args] == ["logits", "labels", "weights", "loss_sum", "counts", "M", "V", "ld", "dtype", "stream"]
    assert [c for c, _ in args] == [ctypes.c_void_p] * 5 + [ctypes.c_int64, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p]
    for fmt in ("bf16", "f16"):
        lib = _lib.load(fmt)
        assert hasattr(lib, "ecamp_ce_eval"), fmt
        # argument errors are reported without a device: nothing is launched
        one = ctypes.c_void_p(16)
        assert lib.ecamp_ce_eval(one, one, one, one, one, 4, 6, 8, 1, None) < 0 and b"multiples of 4" in lib.ecamp_last_error()
        assert lib.ecamp_ce_eval(one, one, one, one, None, 4, 8, 8, 1, None) < 0 and b"null pointer" in lib.ecamp_last_error()
