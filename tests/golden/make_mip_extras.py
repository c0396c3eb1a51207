"""Generates tests/golden/g13_mip_extras.npz: the REFERENCE's own integrate_weights / sorted_interp (mipnerf360/helper.py:196-222,
imported under the stubs of _ref_loader.py) and, for the "sdist" convention, its s_to_t (construct_ray_warps, :168-172), in fp64 and
in fp32, on the inputs of tests/mip_extras_cases.py: both families and both edge conventions, every n up to 129 at nine rays with
the three standard quantiles, and the eight-quantile case.  Build-container only.

Stored as flat arrays, the cases concatenated in the order of mip_extras_cases.fixture_cases() (fixture_case cuts one out again):
"edges" and "w" (fp32) as the entry point receives them, "pct64" (fp64) the reference's percentiles and "pct32_ulps" (int32) its
fp32 percentiles as the distance in units of the last place from the fp64 result rounded to fp32.  Data only.

    python tests/golden/make_mip_extras.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import _ref_loader as ref  # noqa: E402
import mip_extras_cases as M  # noqa: E402


def g13_mip_extras():
    H = ref.load("models.mipnerf360.helper")
    _, s_to_t = H.construct_ray_warps(M.NEAR, M.FAR)
    parts = {"edges": [], "w": [], "pct64": [], "pct32_ulps": []}
    for family, n, convention, u in M.fixture_cases():
        inp = M.inputs(family, n)
        parts["edges"].append(M.kernel_edges(inp, family, convention)[0].numpy().reshape(-1))
        parts["w"].append(inp["w"].numpy().reshape(-1))
        res = {dtype: M.evaluate(inp, family, convention, u, dtype, interp=H.sorted_interp, integrate=H.integrate_weights,
                                 warp=s_to_t)["pct"] for dtype in (torch.float64, torch.float32)}
        assert res[torch.float64].dtype == torch.float64 and res[torch.float32].dtype == torch.float32
        p64 = res[torch.float64].numpy().reshape(-1)
        parts["pct64"].append(p64)
        parts["pct32_ulps"].append(res[torch.float32].numpy().reshape(-1).view(np.int32) - p64.astype(np.float32).view(np.int32))
    out = {k: np.concatenate(v) for k, v in parts.items()}
    path = os.path.join(HERE, "g13_mip_extras.npz")
    np.savez_compressed(path, **out)
    print("g13_mip_extras %.1f KB, %d arrays" % (os.path.getsize(path) / 1024, len(out)))


if __name__ == "__main__":
    if not ref.reference_available():
        sys.exit("reference tree not found at %s" % ref.REFERENCE_ROOT)
    g13_mip_extras()
