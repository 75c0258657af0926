"""Writes tests/golden/deepseek_moe_modes01.npz: the bits omx_moe_forward gives in modes 0 / 1 (Mixtral, Qwen3-MoE) on the inputs of
tests/test_gpu_deepseek_moe.py.  Recorded on the commit BEFORE the mode-2 router joined the router kernel, so that the test holds the
two older arithmetics to what they computed then.  Run on a GPU from the repository root of that commit (with this file, and
tests/deepseek_moe_rule.py, copied in):  python tests/golden/make_deepseek_moe_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

if __name__ == "__main__":
    import omx_import
    import deepseek_moe_rule as dr
    omx = omx_import.load_package()
    omx.require_device()
    out = os.environ.get("OMX_GOLDEN_OUT", os.path.join(HERE, "deepseek_moe_modes01.npz"))
    np.savez_compressed(out, **dr.run_modes01(omx))
    print("wrote", out, os.path.getsize(out), "bytes")
