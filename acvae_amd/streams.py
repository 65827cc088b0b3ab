"""Second streams: the one place in the package that orders work across streams and keeps tensors alive for a stream other
than the one they were allocated on (the caching allocator hands a freed block back to its own stream at once).  The rule
is structural: every device tensor handed to a library call that may leave work behind on a second stream is kept for that
stream (``_lib.call_keeping``); what crosses between streams in Python goes through ``beside`` or ``hand_over``."""
import contextlib

import torch

_SCRATCH = {}


def scratch_buffer(nbytes, device, tag=None):
    """Grow-only scratch per (device, stream): contents are dead between library calls, and calls on one stream
    are ordered, so one buffer per stream is enough (the posterior runs on a side stream beside the encoder).  A call
    that leaves work behind on a second stream (acvae_decode_bwd) takes its own buffer (``tag``)."""
    key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream, tag)
    buf = _SCRATCH.get(key)
    if buf is None or buf.numel() < nbytes:
        _SCRATCH[key] = buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
    return buf


def keep(stream, *objs, _seen=None):
    """Keep every device tensor among ``objs`` alive until ``stream`` has passed this point: lists, tuples and dict values
    are walked, ``None`` and whatever is not on a device are skipped, a tensor that occurs twice is recorded once."""
    seen = set() if _seen is None else _seen
    for o in objs:
        if isinstance(o, (list, tuple, dict)):
            keep(stream, *(o.values() if isinstance(o, dict) else o), _seen=seen)
        elif getattr(o, "is_cuda", False) and id(o) not in seen:
            seen.add(id(o))
            o.record_stream(stream)


class SecondStreams:
    """The model's second streams, made on first use per device at the default priority: ``decode``, the decode calls' (prior
    chain forward, trailing parameter gradients backward), and ``posterior``, the posterior's own (forward beside the
    encoder, backward beside that trailing work: on the SAME stream its backward - which the encoder's backward waits for -
    sat behind 0.6 ms of it)."""

    def __init__(self):
        self._made = {}

    def get(self, which, main):
        s = self._made.get(which)
        if s is None or s.device != main.device:
            s = self._made[which] = torch.cuda.Stream(device=main.device)
        return s

    def aux_handle(self):
        """The decode calls' second stream as the raw handle the library takes (``aux_stream``)."""
        return self.get("decode", torch.cuda.current_stream()).cuda_stream


@contextlib.contextmanager
def beside(main, side, *inputs):
    """``with beside(main, side, *inputs) as on_side``: ``side`` waits for what ``main`` holds so far and ``inputs`` are kept
    for it; ``on_side(fn, ...)`` calls ``fn`` with ``side`` current; on leaving, ``main`` waits for ``side`` and every tensor
    of those calls' results is kept for ``main``.  With ``side is main`` nothing is ordered or kept."""
    results = []

    def on_side(fn, *args, **kw):
        with torch.cuda.stream(side):
            results.append(fn(*args, **kw))
        return results[-1]

    if side is not main:
        side.wait_stream(main)
        keep(side, inputs)
    yield on_side
    if side is not main:
        main.wait_stream(side)
        keep(main, results)


def join_after_backward(cur, side, params):
    """Order ``cur`` behind the parameter gradients a backward node left trailing on ``side``: at the end of the pass, where
    their consumers (whoever reads .grad after backward()) are - or now, if some leaf already has a .grad."""
    if any(p is not None and p.is_leaf and p.grad is not None for p in params):   # (a projected embedding table is not a leaf)
        cur.wait_stream(side)                      # autograd will accumulate into .grad on this stream right away
    else:
        torch.autograd.Variable._execution_engine.queue_callback(lambda: cur.wait_stream(side))


def hand_over(tensor, ready):
    """The current stream takes over ``tensor``, filled on another stream in front of that stream's event ``ready``."""
    cur = torch.cuda.current_stream()
    cur.wait_event(ready)
    keep(cur, tensor)
