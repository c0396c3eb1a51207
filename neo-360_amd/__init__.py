"""neo360_amd — MI355X-native implementation of the NeO-360 ray-marching hot path.

Python host code over a C-ABI HIP library (`lib/libneo360_hip.so`, header
`include/neo360_hip.h`).  PyTorch-ROCm supplies device memory, streams and
torch.distributed only; every kernel on the inference path is hand-written HIP for gfx950.
There is no CPU or eager-PyTorch fallback: calls fail loudly if the library is
missing or the tensors are not on a ROCm device.

The differentiable training calls (`training.py`) are chains of the library's operators - samplers, encodings, lookups,
MLP / linear-layer GEMMs and compositing, each with a native backward - held together by torch autograd.  All four renderers run
their MLPs as one fused native chain each way (`nerfpp_mlp*`, `nerf_mlp`, `pixel_mlp_fused`, `mip_mlp_fused`); the per-layer
composition on `training.linear` remains as `module.train_fused = False` and for Mip-NeRF 360 shapes outside the chain's range.
The texel-space projections of the latent run on the library's own GEMM kernels (`neo_linear_*`), not on a BLAS library.
"""
__version__ = "0.1.0"
