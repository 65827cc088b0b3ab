"""The page-locked staging ring (``_lib._PinnedRing``) with real copies behind it: slots are reused lap after lap while the
stream that reads them is held up, so a slot handed out before its copy has passed shows as a device tensor that differs
from its source.  tests/test_pinned_ring_cpu.py holds the bookkeeping itself (and the two-thread interleavings) to account."""
import threading

import pytest
import torch

from acvae_amd import _lib
from test_stream_lifetimes_gpu import stall_cycles

pytestmark = pytest.mark.gpu

RING = 16 << 10
DTYPES = (torch.uint8, torch.int16, torch.int64, torch.float32)


def sources(seed=0):
    """>= 64 host tensors of distinct contents and mixed dtypes, 1 B .. RING / 4 bytes (more than four laps of the ring in all),
    two larger than a quarter of the ring and one empty one (those three bypass it)."""
    g = torch.Generator().manual_seed(seed)
    sizes = [1, 2, 255, 256, 257, RING // 4, RING // 4 - 1, 1000, 3000, 4000] * 7            # bytes
    out = []
    for i, nbytes in enumerate(sizes):
        dt = DTYPES[i % 4] if nbytes >= 8 and nbytes % 8 == 0 else (torch.int16 if nbytes % 2 == 0 else torch.uint8)
        n = nbytes // torch.empty(0, dtype=dt).element_size()
        if dt == torch.float32:
            t = torch.randn(n, generator=g) + i
        else:
            t = torch.randint(0, 120, (n,), generator=g).to(dt) + (i % 7)
        out.append(t)
    out.insert(5, torch.randn(RING // 4 // 4 + 1, generator=g))          # oversize by one element
    out.insert(40, torch.randint(0, 99, (RING,), generator=g).to(torch.uint8))
    out.insert(20, torch.empty(0, 3, dtype=torch.float32))
    assert len(out) >= 64 and sum(t.numel() * t.element_size() for t in out) > 4 * RING
    return out


def send_all(ring, srcs, streams):
    """Stage every source (even ones through ``stage``, odd ones through ``fill``), source i on streams[i % len]."""
    got = []
    for i, t in enumerate(srcs):
        with torch.cuda.stream(streams[i % len(streams)]):
            if i % 2 == 0:
                got.append(ring.stage(t, torch.device("cuda")))
            else:
                got.append(ring.fill(tuple(t.shape), t.dtype, torch.device("cuda"), lambda slot, t=t: slot.copy_(t)))
    return got


@pytest.mark.parametrize("nstreams", [1, 2], ids=["one_stream", "two_streams_alternating"])
def test_ring_wraps_under_a_stalled_stream_without_losing_a_byte(nstreams):
    ring = _lib._PinnedRing(nbytes=RING)
    srcs = sources()
    streams = [torch.cuda.Stream() for _ in range(nstreams)]
    cycles = stall_cycles()
    torch.cuda.synchronize()
    with torch.cuda.stream(streams[0]):
        torch.cuda._sleep(cycles)                         # the one bounded spin: the first lap's copies are pending behind it
    got = send_all(ring, srcs, streams)
    torch.cuda.synchronize()
    for i, (t, d) in enumerate(zip(srcs, got)):
        assert d.is_cuda and d.dtype == t.dtype and d.shape == t.shape, i
        assert torch.equal(d.cpu(), t), f"tensor {i} ({t.dtype}, {t.numel()} elements) arrived changed"
    assert ring.head <= RING and all(ent[1] <= RING for ent in ring.live)


def test_two_host_threads_stage_through_the_shared_device_ring():
    """Two host threads, each on its own stream, stage 300 small distinct tensors each through ``_lib.h2d``, i.e. through the
    ONE ring of the device, and every tensor arrives bit for bit.  This is a smoke test of the ring's lock: it passes on most
    runs without it.  The proof of the race it guards against (an entry appended by one thread while another sits inside
    ``_reserve`` used to be dropped, and its slot handed out again) is the deterministic interleaving in
    tests/test_pinned_ring_cpu.py."""
    dev = torch.device("cuda", torch.cuda.current_device())
    _lib.h2d(torch.zeros(1), dev)                         # the device's ring exists before the threads start
    results, errors = [None, None], []

    def work(k):
        try:
            g = torch.Generator().manual_seed(100 + k)
            srcs = [torch.randn(1 + (7 * i + k) % 600, generator=g) + i for i in range(300)]
            with torch.cuda.stream(torch.cuda.Stream()):
                got = [_lib.h2d(t, dev) for t in srcs]
                torch.cuda.current_stream().synchronize()
            results[k] = (srcs, got)
        except BaseException as exc:       # noqa: BLE001  (re-raised below)
            errors.append(exc)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0]
    torch.cuda.synchronize()
    for k in range(2):
        srcs, got = results[k]
        for i, (t, d) in enumerate(zip(srcs, got)):
            assert torch.equal(d.cpu(), t), (k, i)
