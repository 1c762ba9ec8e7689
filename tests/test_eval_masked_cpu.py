"""not gpu: the host side of masked-token evaluation -- the declaration / export of `ecamp_compact_rows` and its workspace query, the
`--eval_score` flag and `engine_pretrain.eval_scored_rows`, the count the compacted head's row capacity is formed from."""
import argparse
import ctypes
import os

import pytest
import torch


def _parse(argv):
    from ecamp_amd.main_pretrain import get_args_parser
    return argparse.ArgumentParser(parents=[get_args_parser()]).parse_args(argv)


def test_header_declares_compact_rows_and_both_builds_export_it():
    from ecamp_amd import _lib
    if not all(os.path.exists(p) for p in _lib.LIB_PATHS.values()):
        from ecamp_amd import build
        build.build(verbose=False, half="both")
    protos = _lib.parse_header()
    assert "ecamp_compact_rows" in protos and "ecamp_compact_rows_workspace_bytes" in protos
    assert _lib.abi_version_of_header() == 5      # added without touching an existing signature
    ret, args = protos["ecamp_compact_rows_workspace_bytes"]
    assert ret is ctypes.c_int64 and [(c, n) for c, n in args] == [(ctypes.c_int64, "M")]
    ret, args = protos["ecamp_compact_rows"]
    assert ret is ctypes.c_int32
    assert [n for _, n in args] == ["x", "ldx", "labels", "weights", "ids", "mask_id", "M", "cols", "V", "cap", "x_out", "labels_out",
                                    "weights_out", "rows_out", "count_out", "ws", "dtype", "stream"]
    p, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    assert [c for c, _ in args] == [p, i64, p, p, p, i64, i64, i32, i32, i64, p, p, p, p, p, p, i32, p]
    for fmt in ("bf16", "f16"):
        lib = _lib.load(fmt)
        assert hasattr(lib, "ecamp_compact_rows") and hasattr(lib, "ecamp_compact_rows_workspace_bytes"), fmt
        # the workspace grows with the row count, holds at least the one sum, and exists up to the largest M
        sizes = [lib.ecamp_compact_rows_workspace_bytes(M) for M in (0, 1, 256, 257, 300000, 2 ** 31 - 1)]
        assert sizes[0] >= 8 and sizes == sorted(sizes) and sizes[-1] < 2 ** 26
        assert lib.ecamp_compact_rows_workspace_bytes(-1) < 0 and lib.ecamp_compact_rows_workspace_bytes(2 ** 31) < 0
        # argument errors are reported without a device: nothing is launched
        one = ctypes.c_void_p(16)
        assert lib.ecamp_compact_rows(one, 6, one, one, None, 3, 4, 6, 8, 4, one, one, one, one, one, one, 0, None) < 0
        assert b"multiples of 16 bytes" in lib.ecamp_last_error()
        assert lib.ecamp_compact_rows(one, 4, one, one, None, 3, 4, 4, 8, 4, one, one, one, one, one, one, 1, None) < 0     # 4 x 2 bytes
        assert b"multiples of 16 bytes" in lib.ecamp_last_error()
        assert lib.ecamp_compact_rows(one, 8, one, one, None, 3, 4, 8, 8, 4, one, one, one, one, None, one, 0, None) < 0
        assert b"null pointer" in lib.ecamp_last_error()
        assert lib.ecamp_compact_rows(one, 8, one, one, None, 3, 2 ** 31, 8, 8, 4, one, one, one, one, one, one, 0, None) < 0
        assert b"2^31" in lib.ecamp_last_error()


def test_eval_score_flag_parses_defaults_to_all_and_rejects_other_values(capsys):
    from ecamp_amd.main_pretrain import check_eval_args
    assert _parse([]).eval_score == "all"
    assert _parse(["--eval_score", "all"]).eval_score == "all"
    assert _parse(["--eval_score", "masked"]).eval_score == "masked"
    with pytest.raises(SystemExit):
        _parse(["--eval_score", "visible"])
    capsys.readouterr()
    check_eval_args(_parse(["--eval_freq", "1", "--synthetic", "--eval_score", "masked"]))
    check_eval_args(_parse(["--eval_only", "--resume", "c.pth", "--synthetic", "--eval_score", "masked"]))
    with pytest.raises(SystemExit, match="--eval_score"):
        check_eval_args(_parse(["--eval_score", "masked"]))                     # nothing would evaluate
    a = _parse(["--eval_freq", "1", "--synthetic"])
    a.eval_score = "visible"                                                      # (a namespace built by hand)
    with pytest.raises(SystemExit, match="--eval_score"):
        check_eval_args(a)
    # the help text says what each scope scores
    from ecamp_amd.main_pretrain import get_args_parser
    helps = {a.dest: a.help for a in get_args_parser()._actions}
    assert "[MASK]" in helps["eval_score"] and "--eval_score" in helps["eval_freq"] and "masked-token" not in helps["eval_freq"]


def test_eval_scored_rows_counts_on_the_host():
    from ecamp_amd.data import MASK
    from ecamp_amd.engine_pretrain import eval_scored_rows
    from oracle import ecamp_oracle as orc
    from oracle import recipe
    cfg = orc.cfg_tiny()
    V = cfg.bert.vocab_size
    batch = recipe.recipe_batch(cfg, 4, 128, seed=0)
    ids, labels = batch["ids"], batch["labels"]
    assert MASK == 3
    want = int(((ids == 3) & (labels >= 0) & (labels < V)).sum())
    got = eval_scored_rows(batch, "masked", V)
    assert isinstance(got, int) and got == want and 0 < want < 4 * 128
    assert eval_scored_rows(batch, "all", V) == int(((labels >= 0) & (labels < V)).sum()) == 4 * 128
    # labels outside [0, V) are not scored in either scope
    off = dict(batch, labels=labels.clone())
    off["labels"][:, 1::2] = -100
    off["labels"][0, 2] = V
    assert eval_scored_rows(off, "all", V) == int(((off["labels"] >= 0) & (off["labels"] < V)).sum()) < 4 * 128
    assert eval_scored_rows(off, "masked", V) == int(((ids == 3) & (off["labels"] >= 0) & (off["labels"] < V)).sum()) < want
    # a batch without any [MASK]
    plain = dict(batch, ids=torch.where(ids == 3, torch.full_like(ids, 7), ids))
    assert eval_scored_rows(plain, "masked", V) == 0 and eval_scored_rows(plain, "all", V) == 4 * 128
    assert torch.equal(batch["labels"], labels) and torch.equal(batch["ids"], ids)
    with pytest.raises(ValueError):
        eval_scored_rows(batch, "visible", V)


def test_compact_cap_is_whole_granules_and_never_empty():
    from ecamp_amd import hip_ops
    g = hip_ops.COMPACT_GRANULE
    assert g == 256
    assert [hip_ops.compact_cap(n) for n in (0, 1, g - 1, g, g + 1, 5 * g)] == [g, g, g, g, 2 * g, 5 * g]
