"""ctypes binding of libacvae_hip.so, generated from include/acvae_hip.h at import time so that the
Python side can never drift from the C ABI.  There is NO fallback: if the library is missing or a
symbol declared in the header is not exported, importing/using the product path raises."""
import ctypes
import os
import re
import threading

import numpy as np
import torch

from . import streams

_HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(_HERE), "include", "acvae_hip.h")
LIB_PATH = os.path.join(_HERE, "libacvae_hip.so")      # the product library; tools load an A/B build with use_library()

_CT = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double,
       "uint64_t": ctypes.c_uint64}
ERRORS = {-1: "ACVAE_EINVAL (bad dims / null pointer)", -2: "ACVAE_EALIGN (alignment)",
          -3: "ACVAE_EUNSUPPORTED", -4: "ACVAE_EWORKSPACE (workspace too small)"}


def parse_header(path=HEADER):
    """-> {name: (restype, [(argname, ctype)])} for every `int|int64_t acvae_*(...)` prototype, and {enum: value}."""
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = {}
    for m in re.finditer(r"\b(int|int64_t)\s+(acvae_\w+)\s*\(([^)]*)\)\s*;", src):
        ret, name, args = m.group(1), m.group(2), m.group(3).strip()
        alist = []
        if args and args != "void":
            for a in args.split(","):
                a = a.strip()
                if "*" in a:
                    alist.append((a.split("*")[-1].strip(), ctypes.c_void_p))
                else:
                    toks = a.replace("const ", "").split()
                    alist.append((toks[-1], _CT[toks[0]]))
        protos[name] = (_CT[ret], alist)
    enums = {}
    for m in re.finditer(r"enum\s+\w*\s*\{([^}]*)\}", src):
        val = -1
        for item in m.group(1).split(","):
            item = item.strip()
            if not item:
                continue
            if "=" in item:
                k, v = item.split("=")
                val = int(v.strip(), 0)
                enums[k.strip()] = val
            else:
                val += 1
                enums[item] = val
    return protos, enums


PROTOS, ENUMS = parse_header()
_defs = dict(re.findall(r"#define\s+(ACVAE_\w+)\s+(\d+)", open(HEADER).read()))
ENUMS_TEXT_N = int(_defs["ACVAE_TEXT_NPARAMS"])
ENC_NPARAMS = int(_defs["ACVAE_ENC_NPARAMS"])
ENC_BF16 = int(_defs["ACVAE_ENC_BF16"])
FLAG_NO_PERSIST = int(_defs["ACVAE_FLAG_NO_PERSIST"])
FLAG_DEFER_PARAM_GRADS = int(_defs["ACVAE_FLAG_DEFER_PARAM_GRADS"])
FLAG_NO_ATTN_SPLIT = int(_defs["ACVAE_FLAG_NO_ATTN_SPLIT"])
FLAG_TEST_STALL = int(_defs["ACVAE_FLAG_TEST_STALL"])
FLAG_ROLLOUT_GRAD = int(_defs["ACVAE_FLAG_ROLLOUT_GRAD"])
_lib = None


class options:
    """Host-side defaults for the per-call `flags` of the C ABI (the library itself keeps no switch but ACVAE_CONV_WINO, the
    benchmark's and two tests' A/B).  Tests and the A/B tools change them through `with _lib.override(persist=False): ...`;
    the environment variables of the earlier rounds still set the initial values."""
    persist = os.environ.get("ACVAE_DECODE_PERSIST", "1") != "0"      # persistent decode / posterior launches
    defer = os.environ.get("ACVAE_DECODE_DEFER", "1") != "0"          # decode backward: parameter gradients trail on the side stream
    attn_split = True                                                 # split-over-frames attention for few query rows
    test_stall = False                                                # ACVAE_FLAG_TEST_STALL (tests only)


class override:
    """`with override(persist=False): ...` sets options for the block.  The options are process-wide (a backward pass reads
    them on autograd's own thread), so blocks entered from several host threads may overlap: the options are always the
    values from before the first open block with every open block's settings applied in the order they were entered.
    (Restoring "what was there on entering" would let a block that leaves first undo one still open, or a block that
    entered inside another leave that one's values behind for good.)"""
    _lock = threading.Lock()
    _open = []
    _base = None

    def __init__(self, **kw):
        self.kw = kw

    @staticmethod
    def _apply():
        vals = dict(override._base)
        for o in override._open:
            vals.update(o.kw)
        for k, v in vals.items():
            setattr(options, k, v)

    def __enter__(self):
        with override._lock:
            if not override._open:
                override._base = {k: v for k, v in vars(options).items() if not k.startswith("_")}
            override._open.append(self)
            override._apply()
        return self

    def __exit__(self, *exc):
        with override._lock:
            override._open.remove(self)
            override._apply()
        return False


def call_flags(defer=False):
    f = 0
    if not options.persist:
        f |= FLAG_NO_PERSIST
    if not options.attn_split:
        f |= FLAG_NO_ATTN_SPLIT
    if options.test_stall:
        f |= FLAG_TEST_STALL
    if defer and options.defer:
        f |= FLAG_DEFER_PARAM_GRADS
    return f


def use_library(path):
    """Load another build of the library (tools/ab_build.py) instead of the product one.  Explicit and process-wide: must
    be called before the first library call."""
    global LIB_PATH
    if _lib is not None:
        raise RuntimeError("acvae_amd._lib.use_library() must come before the first library call")
    LIB_PATH = os.path.abspath(path)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(the AC-VAE HIP path has no CPU fallback)")
        _lib = ctypes.CDLL(LIB_PATH)
        for name, (ret, args) in PROTOS.items():
            fn = getattr(_lib, name)            # AttributeError if the header declares what the .so lacks
            fn.restype = ret
            fn.argtypes = [t for _, t in args]
    return _lib


def ptr_table(tensors):
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def _conv(x):
    if isinstance(x, torch.Tensor):
        return x.data_ptr()
    if isinstance(x, (list, tuple)):             # a list of tensors / None where the entry takes a pointer table
        return ptr_table(x)
    return x


def current_stream():
    return torch.cuda.current_stream().cuda_stream


def call(name, *args):
    """Call an `int acvae_*` entry point; tensors are passed as device pointers, lists of tensors as pointer tables; raises
    on non-zero."""
    fn = getattr(lib(), name)
    rc = fn(*[_conv(a) for a in args])
    if PROTOS[name][0] is ctypes.c_int and rc != 0:
        what = ERRORS.get(rc, f"hipError_t {rc}" if rc > 0 else f"code {rc}")
        raise RuntimeError(f"{name} failed: {what}")
    return rc


def call_keeping(keep_on, name, *args):
    """call(name, *args) for an entry that may leave work behind on the stream ``keep_on`` when it returns (None: it does
    not): EVERY device tensor among the arguments, the lists behind the tables included, is then kept alive for that stream."""
    try:
        return call(name, *args)
    finally:
        if keep_on is not None:
            streams.keep(keep_on, args)


def grad_buffer(views, p):
    """Where a backward writes p's gradient: p's view of the train step's flat gradient (``views``: {param: view} or None)
    as a fresh alias, which autograd adopts as .grad without a copy, or a new tensor."""
    if views is not None and p in views:
        return views[p].detach()
    return torch.empty_like(p)


# ---- persistent launches: status words (include/acvae_hip.h, acvae_persist_status_register)
_STATUS = {}
_STATUS_NAMES = ("decode forward", "decode backward", "posterior forward", "posterior backward")


def persist_status(dev):
    """The device's status words (page-locked int32[8], registered with the library on first use)."""
    dev = torch.device(dev)
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    t = _STATUS.get(key)
    if t is None:
        t = torch.zeros(8, dtype=torch.int32).pin_memory()
        call("acvae_persist_status_register", key, t.data_ptr())
        _STATUS[key] = t
    return t


def check_persist_status(dev):
    """Raise if a persistent launch on `dev` gave up since the last check.  Meaningful once the streams that carried the
    launches have drained (TrainStep calls it behind its in-flight event); the launch's outputs are NaN either way."""
    t = persist_status(dev)
    if int(t[4]) != 0:
        which = [n for k, n in enumerate(_STATUS_NAMES) if int(t[k]) != 0]
        t.zero_()
        raise RuntimeError("acvae_amd: a persistent launch could not complete (" + ", ".join(which) + "): part of its grid was "
                           "never resident - is another process running persistent kernels on this GPU?  Its outputs were "
                           "overwritten with NaN.  ACVAE_DECODE_PERSIST=0 selects the per-step launches.")


# ---- workspaces of acvae_attn_fwd's split-over-frames form: zeroed once, one per (device, stream)
_ATTN_WS = {}


def attn_fwd_workspace(N, Tq, S, A, E, dev):
    """(tensor or None, bytes) for acvae_attn_fwd on the current stream.  The counters at its head must start zeroed and are
    left zeroed by every call, so the buffer is cached per stream and only re-made (zeroed) when it has to grow."""
    nbytes = call("acvae_attn_fwd_workspace_bytes", N, Tq, S, A, E)
    if nbytes <= 0 or not options.attn_split:
        return None, 0
    dev = torch.device(dev)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), current_stream())
    t = _ATTN_WS.get(key)
    if t is None or t.numel() < nbytes:
        t = torch.zeros(int(nbytes), dtype=torch.uint8, device=dev)
        _ATTN_WS[key] = t
    return t, t.numel()


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("acvae_amd: the HIP path needs tensors on an MI355X device (no CPU fallback)")


class _PinnedRing:
    """One page-locked staging buffer per device, handed out as a ring.  A freshly hipHostMalloc'ed block makes the
    first copy out of it wait for the GPU to drain, and torch's caching host allocator needs a fresh block whenever
    the host runs ahead of the previous copies, so the per-step host->device copies stage through memory that is
    pinned once.  A slot is reused only after the copy that last read it has passed (event), which blocks only when
    the host is a whole ring ahead of the GPU.

    Several host threads may stage through one ring (there is one per device, not per thread).  ``head`` and ``live`` are
    read and written under ``lock`` only.  A slot enters ``live`` the moment it is reserved, without an event yet, so that
    it is never invisible between ``_reserve`` and ``_commit``; whoever is handed an overlapping slot first waits for that
    commit and then for the copy.  All waiting is done with the lock released: a waiter never keeps another thread from
    reserving or committing, and a wait is only ever for an entry reserved earlier, so waits cannot form a cycle."""

    def __init__(self, nbytes=32 << 20):
        self.buf = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        self.head = 0
        self.live = []           # [start, end, event or None (reserved, not sent yet), threading.Event: sent] in allocation order
        self.lock = threading.Lock()

    def _reserve(self, n):
        span = (n + 255) & ~255
        wait = []
        with self.lock:
            if self.head + span > self.buf.numel():
                self.head = 0
            s, e = self.head, self.head + span
            self.head = e
            # every live entry that overlaps the slot must have been copied out (not only the oldest one: after a wrap an
            # old tail entry the new lap never reaches can sit in front of newer ones that do overlap); entries whose copy
            # has already passed are dropped on the way so the list stays short.  An overlapped entry stays listed until
            # it has been waited for: it may reach beyond this slot, into one that another thread is handed meanwhile.
            keep = []
            for ent in self.live:
                if ent[0] < e and ent[1] > s:
                    wait.append(ent)
                    keep.append(ent)
                elif ent[2] is None or not ent[2].query():
                    keep.append(ent)
            keep.append([s, e, None, threading.Event()])
            self.live[:] = keep
        for ent in wait:
            ent[3].wait()                        # reserved by another thread and not sent yet: until it is (or is given up)
            if ent[2] is not None:
                ent[2].synchronize()
        if wait:
            with self.lock:
                self.live[:] = [x for x in self.live if not any(x is w for w in wait)]
        return s, e

    def _commit(self, s, e, ev):
        """The slot [s, e) handed out by ``_reserve`` has been sent and ``ev`` is recorded behind its copy; ``ev=None``: it
        was given up (the producer raised), nothing reads it."""
        with self.lock:
            for i, ent in enumerate(self.live):
                if ent[0] == s and ent[1] == e and ent[2] is None and not ent[3].is_set():
                    if ev is None:
                        del self.live[i]
                    ent[2] = ev
                    ent[3].set()
                    return
        raise RuntimeError(f"pinned ring: no reserved slot [{s}, {e}) to commit")

    def _send(self, slot, s, e, dev):
        out = slot.to(dev, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        self._commit(s, e, ev)
        return out

    def stage(self, t, dev):
        n = t.numel() * t.element_size()
        if n == 0 or n > self.buf.numel() // 4:
            return t.pin_memory().to(dev, non_blocking=True)
        s, e = self._reserve(n)
        try:
            slot = self.buf[s:s + n].view(t.dtype).view(t.shape)
            np.copyto(slot.numpy(), t.numpy())   # plain memcpy: torch's copy_ fans a 1 MB copy out over the intra-op pool
            return self._send(slot, s, e, dev)
        except BaseException:
            self._give_up(s, e)
            raise

    def fill(self, shape, dtype, dev, fill):
        """Reserve a slot, let ``fill(slot_tensor)`` produce the data in place (e.g. torch.randn(..., out=)), send it."""
        n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        if n == 0 or n > self.buf.numel() // 4:
            t = torch.empty(shape, dtype=dtype)
            fill(t)
            return t.pin_memory().to(dev, non_blocking=True)
        s, e = self._reserve(n)
        try:
            slot = self.buf[s:s + n].view(dtype).view(shape)
            fill(slot)
            return self._send(slot, s, e, dev)
        except BaseException:
            self._give_up(s, e)
            raise

    def _give_up(self, s, e):
        """A reserved slot whose producer raised: unless it was sent all the same, nobody must wait for it for ever."""
        try:
            self._commit(s, e, None)
        except RuntimeError:
            pass                                 # (committed before the exception: the entry has its event)


_RINGS = {}
_RINGS_LOCK = threading.Lock()


def _ring(dev):
    """The device's ring, made on first use (once, whichever thread comes first)."""
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    ring = _RINGS.get(key)
    if ring is None:
        with _RINGS_LOCK:
            ring = _RINGS.get(key)
            if ring is None:
                ring = _RINGS[key] = _PinnedRing()
    return ring


def h2d(t, dev, dtype=None):
    """Host array/tensor -> device without stalling the host: a copy out of pageable memory waits until everything
    queued before it has run, so stage through the page-locked ring and copy asynchronously."""
    t = torch.as_tensor(t)
    if t.device.type != "cpu":
        return t.to(device=dev, dtype=dtype)
    if dtype is not None:
        t = t.to(dtype)
    dev = torch.device(dev)
    if dev.type != "cuda":
        raise RuntimeError("acvae_amd: the HIP path needs a GPU device (no CPU fallback)")
    return _ring(dev).stage(t.contiguous(), dev)


def h2d_fill(shape, dtype, dev, fill):
    """Like h2d, but the host data is produced by ``fill(tensor)`` directly in the page-locked staging slot."""
    dev = torch.device(dev)
    if dev.type != "cuda":
        raise RuntimeError("acvae_amd: the HIP path needs a GPU device (no CPU fallback)")
    return _ring(dev).fill(tuple(shape), dtype, dev, fill)
