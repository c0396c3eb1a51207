"""Per-device library context and tensor marshalling helpers."""
import ctypes
import os
import weakref

import torch

from . import _lib

_contexts = {}


class NeoDeviceError(_lib.NeoError, ValueError):
    """A tensor on the wrong device: a NeoError as ever (there is no CPU fallback), and a ValueError like every other breach of
    a tensor contract."""


def _require_gpu(t, name, exc=_lib.NeoError):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise exc(
            "%s is on %s: the neo360_amd path runs only on a ROCm device (there is no CPU fallback)" % (name, t.device))


ALIGN = 16      # bytes: the widest load the kernels make through a pointer of the C ABI (float4)
FLOATS = (torch.float32, torch.float64, torch.float16, torch.bfloat16)


def _shape_text(shapes):
    """'(7, 3) or (7,)': tuples as Python prints them, '*' for an extent that may be anything."""
    return " or ".join("(%s%s)" % (", ".join("*" if e is None else str(int(e)) for e in s), "," if len(s) == 1 else "") for s in shapes)


def _shape_fits(shape, want):
    return len(shape) == len(want) and all(w is None or int(w) == int(e) for e, w in zip(shape, want))


def _readable(t, dtype):
    """t as a dense tensor of `dtype` whose first byte sits on a 16-byte boundary; t itself when it already is one."""
    if t.dtype != dtype:
        t = t.to(dtype)
    if not t.is_contiguous():
        t = t.contiguous()
    if t.data_ptr() % ALIGN:
        t = t.clone(memory_format=torch.contiguous_format)      # a fresh allocation: the allocators align far beyond 16 bytes
    return t


def dense(t, name, shape=None, dtypes=FLOATS, to=torch.float32, device=None, on_device=True):
    """The tensor contract of an entry point, applied to one argument: the dense, `to`-typed, 16-byte-aligned tensor the library
    may read.  It is `t` itself when t already is that (same object: the callers' identity-keyed caches keep working), a copy
    otherwise - of a strided, expanded, transposed or misaligned view, or of another accepted dtype; `t` is never written.

    shape: the expected shape with the caller's symbolic extents already resolved - a tuple whose None entries accept any
    extent, or a list of such tuples (alternatives, e.g. [(R,), (R, 1)]); None checks no shape.  dtypes: the accepted dtypes
    (default: every floating-point type; pass e.g. (torch.int32,) with to=torch.int32 for an index table).  device: the device
    the tensor must be on besides being a ROCm device (the device of the tensor that defines the call's sizes).
    Raises TypeError for a non-tensor, ValueError("<name> must have shape ..., got ...") for a wrong rank or extent,
    ValueError for a dtype outside `dtypes` or another device, and NeoDeviceError (a NeoError and a ValueError) for a tensor that
    is on no ROCm device.  on_device=False switches the device requirements off: for a small table the wrapper reads on the host
    (camera poses), and for the CPU tests of this function."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor, got %s" % (name, type(t).__name__))
    if t.dtype not in dtypes:
        kind = ("a floating-point" if all(d.is_floating_point for d in dtypes) else
                "a bool" if tuple(dtypes) == (torch.bool,) else "an integer (%s)" % ", ".join(str(d) for d in dtypes))
        raise ValueError("%s must be %s tensor, got %r" % (name, kind, t.dtype))
    if shape is not None:
        shapes = [tuple(shape)] if isinstance(shape, tuple) else [tuple(s) for s in shape]
        if not any(_shape_fits(t.shape, s) for s in shapes):
            raise ValueError("%s must have shape %s, got %s" % (name, _shape_text(shapes), tuple(t.shape)))
    if on_device:
        _require_gpu(t, name, NeoDeviceError)
        if device is not None and t.device != device:
            raise ValueError("%s must be on %s, got %s" % (name, device, t.device))
    return _readable(t, to)


def owned_output(t, name, shape, dtype=torch.float32, device=None, on_device=True):
    """A caller-owned output (`out=`, `reuse=`): the library writes THROUGH it, so nothing is converted - a tensor of another
    shape, dtype or device, a strided view or a misaligned one is refused with ValueError (TypeError for a non-tensor)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor, got %s" % (name, type(t).__name__))
    if not _shape_fits(t.shape, tuple(shape)):
        raise ValueError("%s must have shape %s, got %s" % (name, _shape_text([tuple(shape)]), tuple(t.shape)))
    if t.dtype != dtype:
        raise ValueError("%s must be a %s tensor (it is written in place), got %r" % (name, dtype, t.dtype))
    if on_device:
        _require_gpu(t, name, NeoDeviceError)
        if device is not None and t.device != device:
            raise ValueError("%s must be on %s, got %s" % (name, device, t.device))
    if not t.is_contiguous() or t.data_ptr() % ALIGN:
        raise ValueError("%s must be a dense, 16-byte-aligned tensor (it is written in place, never through a copy), got strides %s "
                         "at offset %d" % (name, tuple(t.stride()), t.storage_offset()))
    return t


def ray_rows(rays, keys=("rays_o", "rays_d", "viewdirs"), on_device=True):
    """The (B,3) per-ray tensors of a batch as the library reads them, in the order of `keys`: rays["rays_o"] defines B and the
    device, every other one must be (B,3) on that device (ValueError otherwise); any float dtype, any strides.  on_device=False:
    shapes and dtype classes only (a frame helper that hands the batch on to a module call, which checks the device)."""
    first = dense(rays["rays_o"], "rays_o", (None, 3), on_device=on_device)
    conv = {"rays_o": first}
    for k in keys:
        if k != "rays_o":
            conv[k] = dense(rays[k], k, (first.shape[0], 3), device=first.device if on_device else None, on_device=on_device)
    return tuple(conv[k] for k in keys)


def radii_shapes(B):
    """Pixel radii of B rays: (B,1) as the reference's batches carry them, (B,), or the (1,B) row render._slice cuts."""
    return [(B, 1), (B,), (1, B)]


def f32(t, name="tensor"):
    """Dense, 16-byte-aligned fp32 device tensor (copies only if needed)."""
    _require_gpu(t, name)
    return _readable(t, torch.float32)


def f64(t, name="tensor"):
    _require_gpu(t, name)
    return _readable(t, torch.float64)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def ptr_table(tensors):
    """A C array of the tensors' data pointers (the `const float* const*` tables of the MLP entry points)."""
    arr = (ctypes.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr()
    return arr


def stream_of(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class Context:
    """Owns one `neo_ctx` (packed weights, scene features, workspaces) on one device."""

    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.NeoError("neo360_amd needs a ROCm device, got %s" % self.device)
        self.index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.lib = _lib.load()
        h = ctypes.c_void_p()
        _lib.check(self.lib.neo_ctx_create(self.index, ctypes.byref(h)))
        self.handle = h
        self.uploaded = {}   # slot key -> fingerprint of the parameters packed on the device
        # the context owns device memory (packed weights, scene features, grow-only workspaces: ~5 GB after a 640x480
        # NeO-360 frame): release it when this object is collected, not at interpreter exit
        self._finalizer = weakref.finalize(self, Context._destroy, self.lib, h)

    @staticmethod
    def _destroy(lib, handle):
        try:
            lib.neo_ctx_destroy(handle)
        except Exception:       # interpreter shutdown: the driver frees everything anyway
            pass

    def stream(self):
        return stream_of(self.device)

    def poll_flags(self):
        flags = ctypes.c_uint32(0)
        _lib.check(self.lib.neo_ctx_poll_flags(self.handle, ctypes.byref(flags), self.stream()))
        return flags.value

    def post_flags(self):
        """Enqueue a read-and-clear of the assertion word on the current stream; no synchronisation."""
        _lib.check(self.lib.neo_ctx_post_flags(self.handle, self.stream()))

    def take_flags(self, wait=False):
        """OR of the posted reads that have completed (wait=False) / of all posted reads (wait=True: blocks)."""
        flags, pending = ctypes.c_uint32(0), ctypes.c_int(0)
        _lib.check(self.lib.neo_ctx_take_flags(self.handle, 1 if wait else 0, self.stream(), ctypes.byref(flags),
                                               ctypes.byref(pending)))
        return flags.value

    def sync_count(self):
        """Blocking waits (stream / event synchronisations) the flag calls of this context have issued."""
        n = ctypes.c_uint64(0)
        _lib.check(self.lib.neo_ctx_sync_count(self.handle, ctypes.byref(n)))
        return n.value

    def stream_waits(self):
        """Cross-stream ordering waits this context has inserted (calls arriving on a stream other than the previous call's)."""
        n = ctypes.c_uint64(0)
        _lib.check(self.lib.neo_ctx_stream_waits(self.handle, ctypes.byref(n)))
        return n.value

    def set_lane(self, lane):
        """Scratch lane (0 / 1) the next calls of this context use (neo_ctx_set_lane)."""
        if getattr(self, "_lane", 0) != lane:
            _lib.check(self.lib.neo_ctx_set_lane(self.handle, int(lane)))
            self._lane = lane

    def set_ray_grid(self, width, first_ray=0):
        """Pixel-grid hint for the next whole-frame renders (neo_ctx_set_ray_grid); width 0 removes it."""
        key = (int(width), int(first_ray) if width else 0)
        if getattr(self, "_ray_grid", (0, 0)) != key:
            _lib.check(self.lib.neo_ctx_set_ray_grid(self.handle, key[0], key[1]))
            self._ray_grid = key

    def set_tp_quad(self, mode):
        """Quad order of the NeO-360 pre-projected split evaluators (neo_ctx_set_tp_quad): None / -1 = the library's per-launch
        default, False / 0 = ray-major everywhere, True / 1 = quads of four rays everywhere, 4 / 8 / 16 = that many rays per group
        everywhere.  Bitwise-neutral."""
        code = -1 if mode is None else int(mode)
        if getattr(self, "_tp_quad", -1) != code:
            _lib.check(self.lib.neo_ctx_set_tp_quad(self.handle, code))
            self._tp_quad = code

    def set_precision(self, mode):
        """'f32' (exact fp32 MFMA) or 'f16x3' (fp16 MFMA, hi/lo-split operands, fp32-equivalent)."""
        code = {"f32": 0, "f16x3": 1, 0: 0, 1: 1}[mode]
        _lib.check(self.lib.neo_ctx_set_precision(self.handle, code))

    def set_timing(self, enable):
        _lib.check(self.lib.neo_ctx_set_timing(self.handle, 1 if enable else 0))

    def read_timing(self):
        ms, n, pts, fl = ctypes.c_double(0), ctypes.c_int(0), ctypes.c_double(0), ctypes.c_double(0)
        _lib.check(self.lib.neo_ctx_read_timing(self.handle, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(pts),
                                                ctypes.byref(fl)))
        return ms.value, n.value, pts.value, fl.value

    KERNEL_NAMES = {0: "unspecified", 1: "k_tp_mlp_hp", 2: "k_tp_mlp_hpp", 3: "k_tp_mlp_h", 4: "k_tp_mlp",
                    5: "k_mip_mlp_h<256> (proposal MLP)", 6: "k_mip_mlp_h<1024> (NeRF MLP, fused)",
                    7: "k_mip_ipe_h + 8 x k_mip_gemm_h + k_mip_mlp_h<tail> (NeRF MLP, layer by layer)", 8: "k_mip_mlp",
                    9: "k_pix_mlp"}

    def read_spans(self):
        """Every timed evaluator launch since set_timing(True), in order: [(ms, kernel name, points, algorithmic flops)]."""
        n = ctypes.c_int(0)
        _lib.check(self.lib.neo_ctx_read_spans(self.handle, 0, None, None, None, None, ctypes.byref(n)))
        cap = n.value
        ms, kid = (ctypes.c_double * cap)(), (ctypes.c_int * cap)()
        pts, fl = (ctypes.c_double * cap)(), (ctypes.c_double * cap)()
        _lib.check(self.lib.neo_ctx_read_spans(self.handle, cap, ms, kid, pts, fl, ctypes.byref(n)))
        return [(ms[i], self.KERNEL_NAMES.get(kid[i], str(kid[i])), pts[i], fl[i]) for i in range(min(cap, n.value))]

    def close(self):
        if self.handle:
            self._finalizer.detach()
            self.lib.neo_ctx_destroy(self.handle)
            self.handle = None


_SIDE_STREAMS = {}


class CallOverlap:
    """Lets consecutive whole-chunk calls of one module overlap on the device (round 6, VERDICT r5 task 4).

    The reference renders a frame as 300 `model(chunk)` calls of 1024 rays (neo360/model.py:861-907).  On one stream each
    call's four evaluator launches end on a partly filled machine and the next call cannot start before the last workgroup of
    this one has finished.  Here call i runs on side stream i % 2 with scratch lane i % 2 of the context, so call i + 1's
    kernels fill the CUs call i's tail leaves idle.  Stream semantics towards the CALLER are unchanged:

    * fork: the side stream waits for an event of the caller's stream.  A fresh event is recorded at every call, EXCEPT when
      the call's ray tensors are views of the very tensor objects (weak identity), at the very versions, of the call the last
      fresh event was recorded for, on the same caller stream and with no `out=` write of this library in between - then
      everything these rays depend on was already enqueued before that event and it is reused.  (A fresh event at call
      i + 1 would sit behind the join of call i and serialise the two.)  Any converted / copied input takes a fresh event.
    * join: before the call returns, the caller's stream waits for the call's completion event, so anything enqueued on it
      afterwards sees the outputs - exactly as if the kernels had run there.
    * memory: outputs are allocated under the side stream and `record_stream`-ed to the caller's stream, inputs are
      `record_stream`-ed to the side stream: the caching allocator will not hand a block to another stream while the other
      side may still touch it.
    """

    def __init__(self, device):
        self.device = device
        self.lanes = max(1, min(4, int(os.environ.get("NEO360_LANES", "2"))))      # calls in flight (library scratch lanes: up to 4)
        # ONE set of side streams per device for every module of the process: HIP multiplexes streams onto a few hardware queues
        # in creation order, and two side streams that land on one queue do not overlap at all (measured: a module whose private
        # pair collided ran its chunk loop at 0.85 of the frame rate where another module's pair gave 0.98)
        pool = _SIDE_STREAMS.setdefault(torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device(), [])
        while len(pool) < self.lanes:
            pool.append(torch.cuda.Stream(device))
        self.streams = pool[:self.lanes]
        self.done = [torch.cuda.Event() for _ in range(self.lanes)]
        self.calls = 0
        self.fresh_forks = 0
        self._fork_ev = None
        self._fork_key = None
        self._fork_bases = ()

    def _key(self, raw, conv, cur):
        bases, ks = [], []
        for a, b in zip(raw, conv):
            if a is not b:
                return None, ()
            base = a._base if a._base is not None else a
            bases.append(base)
            ks.append((base._version, a.untyped_storage().data_ptr()))
        return (tuple(ks), cur.cuda_stream, _lib.write_epoch), tuple(bases)

    def begin(self, raw, conv):
        """-> (side stream, lane, caller's stream).  The side stream is ordered behind everything the inputs depend on."""
        cur = torch.cuda.current_stream(self.device)
        lane = self.calls % self.lanes
        self.calls += 1
        side = self.streams[lane]
        key, bases = self._key(raw, conv, cur)
        reuse = (key is not None and key == self._fork_key and len(bases) == len(self._fork_bases)
                 and all(r() is b for r, b in zip(self._fork_bases, bases)))
        if not reuse:
            ev = torch.cuda.Event()
            ev.record(cur)
            self._fork_ev, self._fork_key = ev, key
            self._fork_bases = tuple(weakref.ref(b) for b in bases)
            self.fresh_forks += 1
        side.wait_event(self._fork_ev)
        for t in conv:
            t.record_stream(side)
        return side, lane, cur

    def end(self, lane, cur, outputs):
        """Completion event on the side stream; the caller's stream waits for it; outputs may be used (and freed) there."""
        ev = self.done[lane]
        ev.record(self.streams[lane])
        cur.wait_event(ev)
        for t in outputs:
            t.record_stream(cur)


def get_context(device):
    device = torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    ctx = _contexts.get(idx)
    if ctx is None:
        ctx = _contexts[idx] = Context(torch.device("cuda", idx))
    return ctx


def new_context(device):
    """A private context (own packed weights / scene), e.g. one per nn.Module."""
    return Context(device)
