"""CPU: the C-ABI library builds, loads and exports every symbol include/acvae_hip.h declares
(no compute calls without a GPU)."""
import ctypes
import os

import __graft_entry__ as ge
from acvae_amd import _lib


def test_build_and_symbols():
    ge.build()
    assert os.path.exists(_lib.LIB_PATH)
    protos, _ = _lib.parse_header()
    assert len(protos) >= 10
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in protos:
        assert hasattr(so, name), f"{name} declared in include/acvae_hip.h but not exported"
    assert _lib.lib().acvae_abi_version() == 3


def test_bad_arguments_are_reported_not_thrown():
    lib = _lib.lib()
    # null pointers / bad dims -> negative code, no launch attempted (safe without a GPU)
    assert lib.acvae_reparam_fwd(None, 0, None, 0, None, None, None, 0, None, 0, 4, 4, None) == -1
    assert lib.acvae_gemm_nt(None, 0, None, 0, None, None, 0, 4, 4, 4, 0, None) == -1
    assert lib.acvae_attn_fwd(None, 0, 0, None, None, None, None, None, 0, 0, None, 0, 0, 1, 1, 1, 1, 1, None, 0, None, 0) == -1
    assert lib.acvae_persist_status_register(-1, None) == -1
    # workspace sizes are host arithmetic: 0 where the split-over-frames form never runs, counters + partials where it does
    assert lib.acvae_attn_fwd_workspace_bytes(32, 21, 62, 512, 512) == 0
    assert lib.acvae_attn_fwd_workspace_bytes(16, 1, 187, 512, 512) == 1024 + 16 * 12 * 516 * 4


def test_library_owns_no_device_memory_and_no_behaviour_switches():
    """SURVEY 8(b) Ownership: the caller owns every buffer, workspaces included - no hipMalloc / hipFree (nor the managed /
    async / host-allocating variants) anywhere in csrc/, no process-global acvae_set_* switches in the ABI, and one
    environment variable read in csrc/, ACVAE_CONV_WINO, which is also the only one the header names."""
    import pathlib
    import re
    root = pathlib.Path(__file__).resolve().parents[1]
    banned = re.compile(r"\bhip(Malloc\w*|Free\w*|HostMalloc|HostAlloc|MallocManaged|MemPool\w*)\s*\(")
    for path in sorted((root / "acvae_amd" / "csrc").glob("*")):
        if path.suffix in (".hip", ".h"):
            code = re.sub(r"//[^\n]*", "", path.read_text())
            assert not banned.search(code), f"{path.name} allocates or frees memory"
    protos, _ = _lib.parse_header()
    assert not [n for n in protos if n.startswith("acvae_set_")]
    assert "ACVAE_DEV_LIB" not in (root / "acvae_amd" / "_lib.py").read_text()
    # ... and one environment variable: every getenv( in csrc/ names ACVAE_CONV_WINO (the benchmark's and two tests' A/B)
    reads = []
    for path in sorted((root / "acvae_amd" / "csrc").glob("*")):
        if path.suffix in (".hip", ".h"):
            code = re.sub(r"//[^\n]*", "", path.read_text())
            reads += [(path.name, m.group(1).strip()) for m in re.finditer(r"\bgetenv\s*\(([^)]*)\)", code)]
    assert reads and all(arg == '"ACVAE_CONV_WINO"' for _, arg in reads), reads
    # the header's conventions paragraph says the same: from where it speaks of environment variables to its next item,
    # the only ACVAE_* name is that one
    head = (root / "include" / "acvae_hip.h").read_text()
    conventions = head[head.index("Conventions"):head.index("*/")]
    assert conventions.count("environment variable") == 1
    switches = conventions[conventions.index("environment variable"):]
    switches = switches[:switches.index("\n *   - ")]
    assert set(re.findall(r"ACVAE_\w+", switches)) == {"ACVAE_CONV_WINO"}


def test_second_streams_are_handled_in_one_module():
    """Cross-stream ordering and lifetimes (record_stream, wait_stream, the autograd engine's queue_callback) live in
    acvae_amd/streams.py and nowhere else in the package."""
    import pathlib
    root = pathlib.Path(__file__).resolve().parents[1]
    files = sorted((root / "acvae_amd").glob("*.py"))
    assert (root / "acvae_amd" / "streams.py") in files
    for path in files:
        src = path.read_text()
        found = [w for w in ("record_stream", "wait_stream(", "queue_callback") if w in src]
        if path.name == "streams.py":
            assert len(found) == 3, found
        else:
            assert not found, f"{path.name} uses {found}: that belongs in acvae_amd/streams.py"


class _FakeTensor:
    def __init__(self, is_cuda=True):
        self.is_cuda, self.recorded = is_cuda, []

    def record_stream(self, stream):
        self.recorded.append(stream)


def test_keep_walks_containers_and_records_each_device_tensor_once():
    from acvae_amd import streams
    a, b, c, d, e = (_FakeTensor() for _ in range(5))
    host = _FakeTensor(is_cuda=False)
    stream = object()
    streams.keep(stream, a, None, [b, None, (c, [d])], {"x": e, "y": None, "z": host, "n": 3}, host, 7, "text", 1.5,
                 (ctypes.c_int * 2)(1, 2))
    for t in (a, b, c, d, e):
        assert t.recorded == [stream]
    assert host.recorded == []
    # the same tensor several times in one call (a parameter in two tables): once
    f = _FakeTensor()
    streams.keep(stream, f, [f, (f,)], {"k": f})
    assert f.recorded == [stream]
    # ... and again by the next call
    streams.keep(stream, [f])
    assert f.recorded == [stream, stream]
    streams.keep(stream)                       # nothing to keep
    # _lib.call hands its whole argument list over: (checked here without a launch, through the same function)
    g, h = _FakeTensor(), _FakeTensor()
    streams.keep(stream, ([g, None], h, 4, None))
    assert g.recorded == [stream] and h.recorded == [stream]


def test_product_never_reaches_into_the_oracle():
    """oracle/ is test infrastructure: nothing under acvae_amd/ may import, load or execute it (only tests/,
    __graft_entry__.smoke() and bench.py's cpu_baseline leg may), and the product has no CPU code path to fall back to."""
    import ast
    import pathlib
    root = pathlib.Path(__file__).resolve().parents[1]
    banned = {"acvae_oracle", "host_oracle", "ref_shim", "make_golden", "oracle"}
    for path in sorted((root / "acvae_amd").rglob("*.py")):
        src = path.read_text()
        for node in ast.walk(ast.parse(src)):
            names = []
            if isinstance(node, ast.Import):
                names = [a.name for a in node.names]
            elif isinstance(node, ast.ImportFrom):
                names = [node.module or ""]
            assert not any(n.split(".")[0] in banned for n in names), f"{path} imports {names}"
        assert "oracle" not in src.lower().replace("the oracle", "").replace("oracle's", ""), f"{path} mentions oracle/"
    for path in sorted((root / "acvae_amd" / "csrc").glob("*")):
        if path.suffix in (".hip", ".h"):
            assert "oracle" not in path.read_text().lower(), f"{path} mentions the oracle"


def test_product_refuses_cpu_tensors():
    """No CPU fallback: the host-side mirrors fail loudly when handed CPU tensors instead of computing on the host."""
    import numpy as np
    import pytest
    import torch
    from acvae_amd.encoder import Cnn10
    enc = Cnn10(64, 512)
    with pytest.raises(RuntimeError, match="no CPU fallback|MI355X|cuda|GPU"):
        enc(torch.zeros(1, 64, 64), np.array([64]))


def test_hot_kernels_keep_everything_in_registers():
    """The persistent decode / posterior kernels and the Winograd kernels run one workgroup per CU at (or near) the 256-register
    limit: a register the compiler cannot place goes to scratch memory, i.e. a global-memory round trip inside the step loop
    (round 3 shipped decode_persist_bwd_kernel with 28 B per lane of it).  The build keeps hipcc's per-kernel resource remarks
    (-Rpass-analysis=kernel-resource-usage) beside every object file; any scratch in these kernels fails here."""
    from acvae_amd import build as b
    ge.build()
    usage = b.resource_usage()
    hot = ("decode_persist_kernel", "decode_persist_bwd_kernel", "posterior_persist_fwd_kernel", "posterior_persist_bwd_kernel",
           "conv_wino_kernel", "conv_wino_bnred_kernel", "conv_wino_stats_kernel", "conv_wino_act_kernel", "conv_wino_wgrad_kernel_s1", "conv_wino_wgrad_kernel_s2",
           "conv_wino_wgrad_kernel_s3", "conv_wino_wgrad_kernel_s4")
    for k in hot:
        hits = {n: u for n, u in usage.items() if k + "E" in n or n.endswith(k)}
        assert hits, f"{k}: no resource record (rebuild with python -m acvae_amd.build --force)"
        for n, u in hits.items():
            assert u.get("scratch", -1) == 0, f"{n}: {u.get('scratch')} bytes per lane of scratch"
            assert u.get("vgprs", 999) <= 256, (n, u)


def test_overlapping_overrides_from_two_threads_restore_the_defaults():
    """Two host threads each run a step under `_lib.override(...)` (test_decode_persist_gpu.py does, with two models on two
    streams); their blocks overlap: A enters, B enters, A leaves, B leaves.  B saw A's value on entry, so restoring "what
    was there on entry" left the option at A's value after both had left - and every later step in the process silently
    ran without the split-over-frames attention.  Once the last override has left, the options are the defaults again,
    whichever order the blocks leave in."""
    import threading
    defaults = (_lib.options.persist, _lib.options.defer, _lib.options.attn_split)
    for b_leaves_first in (False, True):
        a_in, b_in, a_out = threading.Event(), threading.Event(), threading.Event()
        seen = {}

        def a():
            with _lib.override(attn_split=False, persist=not defaults[0]):
                a_in.set()
                b_in.wait(10)
                if b_leaves_first:
                    a_out.wait(10)
            a_out.set()

        def b():
            a_in.wait(10)
            with _lib.override(attn_split=False, defer=not defaults[1]):
                b_in.set()
                if not b_leaves_first:
                    a_out.wait(10)
                seen["inside"] = (_lib.options.attn_split, _lib.options.defer)
            if b_leaves_first:
                seen["a_still_in"] = (_lib.options.attn_split, _lib.options.persist)
                a_out.set()

        ts = [threading.Thread(target=f) for f in (a, b)]
        [t.start() for t in ts]; [t.join(20) for t in ts]
        assert seen["inside"] == (False, not defaults[1])
        if b_leaves_first:                     # A's block is still open: its values hold
            assert seen["a_still_in"] == (False, not defaults[0])
        assert (_lib.options.persist, _lib.options.defer, _lib.options.attn_split) == defaults, b_leaves_first
