"""The page-locked staging ring behind every ``_lib.h2d`` / ``h2d_fill`` (``_lib._PinnedRing``), without a device: rings are
built with ``object.__new__`` over a plain buffer and events are fakes with ``query()`` / ``synchronize()``.

What the ring owes its callers: a slot handed out by ``_reserve`` overlaps no earlier slot whose copy may still be read.
An earlier slot is safe once its event has completed or ``_reserve`` itself has synchronised it (or, for a slot another
thread has reserved and not sent yet, once that thread has committed it and the event has passed).  The model-based test
walks random histories through one thread; the interleaving tests park one thread inside ``_reserve`` while another
performs a whole reserve + commit, which is where entries used to be lost."""
import random
import threading

import numpy as np
import pytest
import torch

from acvae_amd import _lib

WAIT = 20.0          # safety net of every cross-thread wait (seconds): a correct run never comes near it


class FakeEvent:
    """torch.cuda.Event as the ring uses it.  ``done``: the copy has passed; ``synced``: ``synchronize()`` was called (which
    also completes it, as waiting for a real event does).  ``on_sync`` / ``on_query`` run first: the interleaving hooks."""

    def __init__(self, done=False, on_sync=None, on_query=None):
        self.done, self.synced = done, False
        self.on_sync, self.on_query = on_sync, on_query

    def query(self):
        if self.on_query is not None:
            hook, self.on_query = self.on_query, None
            hook()
        return self.done

    def synchronize(self):
        if self.on_sync is not None:
            hook, self.on_sync = self.on_sync, None
            hook()
        self.synced = self.done = True


class SpyLock:
    """A lock that tells when somebody had to wait for it (``progress``, which a test also sets when the other thread is
    through): lets a test park a thread that holds the lock until another thread has either finished or is provably
    blocked on it, without any sleep."""

    def __init__(self):
        self._lock = threading.Lock()
        self.progress = threading.Event()

    def acquire(self, blocking=True, timeout=-1):
        if self._lock.acquire(False):
            return True
        if not blocking:
            return False
        self.progress.set()
        return self._lock.acquire(True, timeout)

    def release(self):
        self._lock.release()

    def __enter__(self):
        self.acquire()
        return self

    def __exit__(self, *exc):
        self.release()


def new_ring(nbytes):
    ring = object.__new__(_lib._PinnedRing)
    ring.buf = torch.zeros(nbytes, dtype=torch.uint8)
    ring.head = 0
    ring.live = []
    ring.lock = SpyLock()
    return ring


def tracked(ring, ev):
    return any(ent[2] is ev for ent in ring.live)


def overlap(a, b):
    return a[0] < b[1] and b[0] < a[1]


# ---------------------------------------------------------------------------------------------- one thread, random history
@pytest.mark.parametrize("nbytes,seed", [(1024, 0), (2048, 1), (4096, 2), (4096, 3)])
def test_random_histories_never_hand_out_a_slot_that_is_still_read(nbytes, seed):
    rng = random.Random(seed)
    ring = new_ring(nbytes)
    history = []                                          # (s, e, event) of every reservation so far
    wraps = 0
    for step in range(3000):
        pending = [h for h in history if not h[2].done]
        if pending and rng.random() < 0.35:
            rng.choice(pending)[2].done = True            # a copy passes, in any order (several streams)
            continue
        n = rng.choice([1, 255, 256, 257, nbytes // 4, rng.randint(1, nbytes // 4)])
        head_before = ring.head
        s, e = ring._reserve(n)
        assert s % 256 == 0 and e % 256 == 0 and e - s >= n and e - s < n + 256
        assert 0 <= s < e <= ring.buf.numel()
        wraps += s < head_before
        for hs, he, hev in history:
            if not hev.done:                              # incomplete and never synchronised (synchronize() completes it)
                assert not overlap((s, e), (hs, he)), (step, (s, e), (hs, he))
        ev = FakeEvent()
        ring._commit(s, e, ev)
        history = [h for h in history if not h[2].done] + [(s, e, ev)]      # (a completed one never matters again)
        # the bookkeeping: nothing listed twice, nothing completed left behind, incomplete entries pairwise disjoint, and
        # therefore never more entries than the ring has 256-byte slots
        assert len({id(ent) for ent in ring.live}) == len(ring.live)
        assert sum(ent[2] is ev for ent in ring.live) == 1
        others = [ent for ent in ring.live if ent[2] is not ev]
        assert all(ent[2] is not None and not ent[2].done for ent in others), step
        spans = sorted((ent[0], ent[1]) for ent in ring.live)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), (step, spans)
        assert len(ring.live) <= nbytes // 256
    assert wraps > 100


def test_wrap_waits_for_the_entries_it_overlaps_behind_an_old_tail_entry_it_does_not_reach():
    """An old entry at the ring's tail that the new lap does not reach sits in front of newer ones that it does overlap: the
    oldest entry is not the only one to look at."""
    ring = new_ring(1024)
    evs = []
    for n in (256, 256, 256, 256):
        s, e = ring._reserve(n)
        evs.append(FakeEvent())
        ring._commit(s, e, evs[-1])
    evs[0].done = evs[1].done = True                      # [0, 512) has passed, [512, 768) and the tail [768, 1024) have not
    assert ring._reserve(256) == (0, 256)
    a = FakeEvent()
    ring._commit(0, 256, a)
    assert ring._reserve(200) == (256, 512)
    b = FakeEvent()
    ring._commit(256, 512, b)
    assert not evs[2].synced and not evs[3].synced and tracked(ring, evs[2]) and tracked(ring, evs[3])
    assert not tracked(ring, evs[0]) and not tracked(ring, evs[1])
    # live is now [512,768) [768,1024) [0,256) [256,512); 600 bytes do not fit behind head = 512: the lap starts over at 0,
    # spans [0, 768) and never reaches the tail entry listed in front of the two it overlaps
    assert ring._reserve(600) == (0, 768)
    assert a.synced and b.synced and evs[2].synced and not evs[3].synced
    assert tracked(ring, evs[3]) and not tracked(ring, a) and not tracked(ring, b) and not tracked(ring, evs[2])


def test_a_reservation_that_fills_the_whole_ring_and_sizes_off_the_alignment():
    ring = new_ring(1024)
    assert ring._reserve(1) == (0, 256)
    one = FakeEvent()
    ring._commit(0, 256, one)
    assert ring._reserve(1024) == (0, 1024)               # exactly the ring: wraps to 0 and waits for everything
    assert one.synced and ring.head == 1024
    whole = FakeEvent()
    ring._commit(0, 1024, whole)
    assert ring._reserve(257) == (0, 512)                 # 257 -> two slots; the ring is full, so from 0 again
    assert whole.synced
    ring._commit(0, 512, FakeEvent())
    assert ring._reserve(255) == (512, 768)
    ring._commit(512, 768, FakeEvent())
    assert ring._reserve(1023) == (0, 1024)
    assert [ent[:2] for ent in ring.live] == [[0, 1024]]


def test_a_slot_given_up_is_forgotten_and_commit_refuses_what_was_not_reserved():
    ring = new_ring(1024)
    s, e = ring._reserve(100)
    ring._commit(s, e, None)
    assert ring.live == []
    with pytest.raises(RuntimeError):
        ring._commit(s, e, FakeEvent())


# ---------------------------------------------------------------------------------------------- two threads, fixed interleaving
def _run_two(ring, a_body, b_body):
    """Thread A runs a_body, thread B runs b_body; exceptions of either are re-raised here."""
    errors = []

    def guard(body):
        def run():
            try:
                body()
            except BaseException as exc:       # noqa: BLE001  (reported below)
                errors.append(exc)
        return run

    ta, tb = threading.Thread(target=guard(a_body)), threading.Thread(target=guard(b_body))
    ta.start(); tb.start()
    ta.join(WAIT); tb.join(WAIT)
    assert not ta.is_alive() and not tb.is_alive(), "a thread never finished"
    if errors:
        raise errors[0]


def test_an_entry_appended_while_another_thread_waits_inside_reserve_is_kept():
    """Thread A wraps and has to wait for the copy out of [0, 256); while it sits in that event's synchronize() (a real
    one releases the GIL), thread B reserves [256, 512) and commits its pending copy.  B's entry must still be tracked when
    both have finished, and the next reservation that overlaps B's slot must synchronise B's event before it returns."""
    ring = new_ring(1024)
    a_parked, b_done = threading.Event(), threading.Event()
    got = {}

    def park():
        a_parked.set()
        assert b_done.wait(WAIT), "B never finished its reserve + commit while A waited for an event"

    old = FakeEvent(on_sync=park)
    assert ring._reserve(256) == (0, 256)
    ring._commit(0, 256, old)
    ring.head = 1024                                      # (the ring was used up to its end since: A's reservation wraps)
    ev_b = FakeEvent()

    def a_body():
        got["a"] = ring._reserve(256)

    def b_body():
        assert a_parked.wait(WAIT)
        got["b"] = ring._reserve(256)
        ring._commit(*got["b"], ev_b)
        b_done.set()

    _run_two(ring, a_body, b_body)
    assert got == {"a": (0, 256), "b": (256, 512)}
    assert old.synced
    assert tracked(ring, ev_b), "B's pending copy is no longer tracked: its slot can be handed out while it is read"
    ring._commit(*got["a"], FakeEvent())
    ring.head = 1024
    assert ring._reserve(512) == (0, 512)
    assert ev_b.synced, "a slot over B's pending copy was handed out without waiting for it"


def test_two_threads_never_get_overlapping_slots_and_both_stay_tracked():
    """The same with thread A parked in an event's query(), i.e. inside the section that reads and advances ``head`` and
    rebuilds ``live``: B either waits for A to leave that section or runs beside it; either way the two slots are
    disjoint, both are tracked afterwards, and a later lap waits for both."""
    ring = new_ring(1024)
    a_parked, b_started = threading.Event(), threading.Event()
    got = {}

    def park():
        a_parked.set()
        assert b_started.wait(WAIT)
        # until B is through, or is provably blocked on the ring's lock (which A holds here)
        assert ring.lock.progress.wait(WAIT), "B neither finished nor blocked"

    far = FakeEvent(on_query=park)                        # a pending copy at the tail that A's slot does not overlap
    ring.head = 768
    assert ring._reserve(256) == (768, 1024)
    ring._commit(768, 1024, far)
    ring.head = 0
    ev_a, ev_b = FakeEvent(), FakeEvent()

    def a_body():
        got["a"] = ring._reserve(256)
        ring._commit(*got["a"], ev_a)

    def b_body():
        assert a_parked.wait(WAIT)
        b_started.set()
        got["b"] = ring._reserve(256)
        ring._commit(*got["b"], ev_b)
        ring.lock.progress.set()

    _run_two(ring, a_body, b_body)
    assert not overlap(got["a"], got["b"]), got
    assert sorted(got.values()) == [(0, 256), (256, 512)]
    assert tracked(ring, ev_a) and tracked(ring, ev_b) and tracked(ring, far)
    ring.head = 1024
    assert ring._reserve(1024) == (0, 1024)
    assert ev_a.synced and ev_b.synced and far.synced


def test_a_slot_reserved_and_not_yet_sent_is_waited_for():
    """Between ``_reserve`` and ``_commit`` a thread copies into its slot.  Another thread that laps the ring meanwhile
    and is handed an overlapping slot must wait for that commit and then for the copy."""
    ring = new_ring(1024)
    got, ev_a = {}, FakeEvent()
    b_waiting = threading.Event()
    got["a"] = ring._reserve(256)                         # A holds [0, 256), not sent yet
    assert ring.live[0][2] is None

    def b_body():
        ring.head = 1024
        b_waiting.set()
        got["b"] = ring._reserve(256)                     # [0, 256) again
        got["a_synced_when_b_returned"] = ev_a.synced

    def a_body():
        assert b_waiting.wait(WAIT)
        ring._commit(*got["a"], ev_a)

    _run_two(ring, a_body, b_body)
    assert got["b"] == (0, 256) and got["a_synced_when_b_returned"]
    assert not tracked(ring, ev_a) and [ent[:3] for ent in ring.live] == [[0, 256, None]]


# ---------------------------------------------------------------------------------------------- stage / fill on a CPU "device"
@pytest.fixture
def cpu_ring(monkeypatch):
    ring = new_ring(4096)
    sent = []

    def send(slot, s, e, dev):
        sent.append((s, e))
        ring._commit(s, e, FakeEvent(done=True))
        return slot.clone()

    monkeypatch.setattr(ring, "_send", send, raising=False)
    ring.sent = sent
    return ring


CONTENTS = [
    torch.arange(-7, 30, dtype=torch.int16),
    torch.arange(5, dtype=torch.int64) * (1 << 40) - 3,
    torch.arange(251, dtype=torch.uint8).reshape(251, 1),
    torch.linspace(-1, 1, 77, dtype=torch.float32).reshape(7, 11),
    torch.tensor(3.25, dtype=torch.float32),              # 0-d
    torch.tensor(-9, dtype=torch.int64),
]


def test_stage_and_fill_keep_contents_for_every_dtype_and_shape(cpu_ring):
    for rep in range(40):                                 # several laps of the 4 KiB ring
        for t in CONTENTS:
            want = t + rep if t.dtype != torch.uint8 else t
            out = cpu_ring.stage(want, "cpu")
            assert out.dtype == want.dtype and out.shape == want.shape and torch.equal(out, want)
            out = cpu_ring.fill(tuple(t.shape), t.dtype, "cpu", lambda slot: slot.copy_(want))
            assert out.dtype == want.dtype and out.shape == want.shape and torch.equal(out, want)
    assert len(cpu_ring.sent) == 40 * len(CONTENTS) * 2
    assert all(e <= 4096 and s % 256 == 0 for s, e in cpu_ring.sent)
    assert sum(1 for a, b in zip(cpu_ring.sent, cpu_ring.sent[1:]) if b[0] < a[0]) >= 4
    assert all(ent[2].done for ent in cpu_ring.live)


def test_h2d_makes_a_non_contiguous_input_contiguous_before_staging(cpu_ring, monkeypatch):
    monkeypatch.setitem(_lib._RINGS, 0, cpu_ring)
    Dev = lambda: torch.device("cuda", 0)     # h2d refuses anything but a GPU device; the ring behind it is the CPU one above
    base = torch.arange(60, dtype=torch.float32).reshape(6, 10)
    for view in (base.t(), base[::2, 1::3], base[:, 3]):
        assert not view.is_contiguous()
        out = _lib.h2d(view, Dev())
        assert out.is_contiguous() and torch.equal(out, view)
    out = _lib.h2d(base.t(), Dev(), torch.int16)
    assert out.dtype == torch.int16 and torch.equal(out, base.t().to(torch.int16))
    out = _lib.h2d_fill((3, 5), torch.int64, Dev(), lambda slot: slot.fill_(7))
    assert out.dtype == torch.int64 and torch.equal(out, torch.full((3, 5), 7))


class _Oversize(torch.Tensor):
    """A CPU tensor whose pin_memory() / to() are counted instead of asking for page-locked memory or a device."""
    calls = []

    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    def pin_memory(self):
        _Oversize.calls.append("pin_memory")
        return self

    def to(self, *a, **k):
        _Oversize.calls.append(("to", a, k))
        return self.as_subclass(torch.Tensor).clone()


@pytest.mark.parametrize("shape,dtype", [((0,), torch.float32), ((3, 0, 2), torch.int64),       # n == 0
                                         ((1025,), torch.uint8), ((300,), torch.float32)])      # n > buf / 4 = 1024
def test_empty_and_oversize_tensors_bypass_the_ring(cpu_ring, shape, dtype, monkeypatch):
    """The ``n == 0`` and ``n > buf / 4`` branches: page-locked memory of their own, no slot."""
    _Oversize.calls = []
    src = torch.arange(int(np.prod(shape)), dtype=torch.float64).reshape(shape).to(dtype)
    out = cpu_ring.stage(_Oversize(src), "gpu0")
    assert _Oversize.calls[0] == "pin_memory" and _Oversize.calls[1] == ("to", ("gpu0",), {"non_blocking": True})
    assert torch.equal(out, src) and cpu_ring.sent == [] and cpu_ring.head == 0 and cpu_ring.live == []
    # fill(): the branch allocates its own tensor, so its pin_memory / to are patched where it makes it
    _Oversize.calls = []
    real_empty = torch.empty
    with monkeypatch.context() as m:
        m.setattr(_lib.torch, "empty", lambda *a, **k: _Oversize(real_empty(*a, **k)) if a and a[0] == shape
                  else real_empty(*a, **k))
        out = cpu_ring.fill(shape, dtype, "gpu0", lambda t: t.copy_(src))
    assert _Oversize.calls == ["pin_memory", ("to", ("gpu0",), {"non_blocking": True})]
    assert torch.equal(out, src) and out.dtype == dtype and cpu_ring.head == 0 and cpu_ring.live == []


def test_the_largest_tensor_that_still_goes_through_the_ring(cpu_ring):
    src = torch.arange(1024, dtype=torch.int64).to(torch.uint8)          # exactly buf / 4
    assert torch.equal(cpu_ring.stage(src, "cpu"), src) and cpu_ring.sent == [(0, 1024)]


def test_a_fill_that_raises_leaves_no_slot_behind(cpu_ring):
    def boom(slot):
        raise ValueError("producer failed")
    with pytest.raises(ValueError):
        cpu_ring.fill((8,), torch.float32, "cpu", boom)
    assert cpu_ring.live == []
    t = torch.arange(8.0)
    assert torch.equal(cpu_ring.stage(t, "cpu"), t)
