"""Child process of tests/test_gpu_dense_mlp_sweep.py: evaluates the vanilla case table in the split arithmetic and writes the
outputs to an .npz.  $NEO_VANILLA_H_WAVES / $NEO_VANILLA_H_TILE select the kernel and are read once per process, which is why
this runs in a process of its own.  Usage: python dense_mlp_child.py OUT.npz"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE, os.path.join(HERE, "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

import dense_mlp_cases as D
from neo360_amd import models, synth


def main(out_path):
    torch.set_grad_enabled(False)
    net = models.NeRF().to("cuda")
    net.precision = "f16x3"
    net.load_state_dict(synth.vanilla_state(0))
    out = {}
    for shape in D.VANILLA_SHAPES:
        inp = {k: v.to("cuda") for k, v in D.vanilla_inputs(*shape).items()}
        for prefix, level in D.VANILLA_LEVELS:
            out["%s%s" % (prefix, D.shape_id(shape))] = net.eval_mlp(level, inp["rays_o"], inp["dirs"], inp["t"]).cpu().numpy()
    net.close()
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
