#!/usr/bin/env python3
"""bench.py's protocol -- same batch, steps, warm-up, timing and JSON result line -- on a model built with ECAMP(f32_residual=True):
the cost of the f32 residual stream against `python bench.py` with the same arguments on the same box.

    python tools/bench_f32_residual.py --gpus 1 --steps 50 --warmup 10 [--dtype fp16]

One GPU only (bench.py's multi-GPU form relaunches itself, without this switch)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ecamp_amd.module import model_ecamp  # noqa: E402

_ecamp = model_ecamp.ecamp


def _ecamp_f32_residual(**kw):
    kw.setdefault("f32_residual", True)
    return _ecamp(**kw)


if __name__ == "__main__":
    a = sys.argv[1:]
    if "--gpus" in a and a[a.index("--gpus") + 1] != "1":
        raise SystemExit("tools/bench_f32_residual.py runs on one GPU (--gpus 1)")
    model_ecamp.ecamp = _ecamp_f32_residual
    import bench
    print("[bench_f32_residual] ECAMP(f32_residual=True)", flush=True)
    sys.argv[0] = bench.__file__
    bench.main()
