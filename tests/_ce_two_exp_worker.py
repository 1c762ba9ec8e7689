"""Child process of tests/test_report_kernels_gpu.py::test_two_exp_register_kernels_in_a_child_process: started with ECAMP_CE_KERNEL=0,
so that ecamp_ce_fwd_bwd takes ce_fwd_bwd_reg_kernel<8> (V <= 16384) and <16> (above) on the bfloat16 build, and holds them to the
cases and the judge of tests/_report_ref.py.  Prints the judge's lines; exit status 1 on a violation."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import _report_ref as R  # noqa: E402


def main():
    assert os.environ.get("ECAMP_CE_KERNEL") == "0", "the parent sets ECAMP_CE_KERNEL=0"
    from ecamp_amd import _lib, hip_ops
    _lib.set_half("bf16")
    dev = torch.device("cuda:0")
    bad = []
    for V in R.V_TWO_EXP:
        x, labels, w = R.ce_case(V, R.BF16, seed=6)
        xd, loss = x.to(dev, torch.bfloat16), torch.zeros(1, device=dev)
        hip_ops.ce_fwd_bwd_(xd, labels.to(dev), w.to(dev), loss)
        torch.cuda.synchronize()
        lines, b = R.ce_judge("two-exp reg<%d> bf16 V=%d" % (8 if V <= 16384 else 16, V), R.BF16, x, labels, w, 1.0, xd.cpu(), loss.item())
        print("\n".join(lines), flush=True)
        bad += b
    if bad:
        print("\n".join(bad), flush=True)
        sys.exit(1)


if __name__ == "__main__":
    main()
