"""GPU: every device tensor handed to acvae_decode_bwd stays out of the allocator's free lists while the decode calls'
second stream still has the call's trailing parameter-gradient work in front of it.

The rule (acvae_amd/streams.py, ``_lib.call_keeping``) is read off the allocator's own state instead of hoping for
a race: the second stream is stalled by a bounded spin in front of backward(), so when backward() has returned on the host
and autograd has dropped its references, the trailing work has provably not run yet.  A tensor argument whose block is
"inactive" at that moment (free for reuse by the stream that allocated it) was not kept; one that is still allocated, or
freed and waiting for the streams recorded on it, is fine.  The gradients are then compared bit for bit with the same step
on one stream.

No bf16 parameter: bf16 changes only the encoder, and the encoder leaves nothing on a second stream."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest
import torch

from acvae_amd import _lib
from test_fullsize_gpu import build as build_no_ln
from test_model_gpu import build_model, hip_loss

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import acvae_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

STALL_MS, STALL_MAX_MS = 50.0, 100.0
_spin = {}


def stall_cycles():
    """torch.cuda._sleep's argument for about STALL_MS, never more than STALL_MAX_MS.  Sized from the device's reported clock
    rate (hipDeviceAttributeClockRate, kHz = cycles per millisecond; torch's device properties do not carry it).  The counter
    the spin kernel reads need not tick at that rate, so one spin of nominally 1 ms is timed once per process and the figure
    is scaled by what it took."""
    if "cycles" not in _spin:
        hip, khz = ctypes.CDLL("libamdhip64.so"), ctypes.c_int(0)
        rc = hip.hipDeviceGetAttribute(ctypes.byref(khz), 5, torch.cuda.current_device())       # 5: ...ClockRate
        if rc != 0:
            hip.hipGetLastError()                # (the runtime keeps the error for the next caller otherwise)
        assert rc == 0 and khz.value > 0, (rc, khz.value)
        per_ms = khz.value
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1)                     # (the first launch loads the spin kernel: not part of the timing)
        torch.cuda.synchronize()
        t0.record(); torch.cuda._sleep(per_ms); t1.record()
        torch.cuda.synchronize()
        took = max(float(t0.elapsed_time(t1)), 1e-3)
        print(f"spin of {per_ms} cycles (1 ms by the reported clock rate) took {took:.3f} ms")
        assert took <= STALL_MAX_MS, f"the calibration spin alone took {took:.1f} ms"
        _spin["cycles"] = int(per_ms / took * STALL_MS)
    return _spin["cycles"]


def device_tensors(args):
    """Every device tensor among a library call's arguments, the lists behind the pointer tables included."""
    for a in args:
        if isinstance(a, (list, tuple)):
            yield from device_tensors(a)
        elif isinstance(a, torch.Tensor) and a.is_cuda:
            yield a


def block_states():
    """[(address, size, state)] of every block the caching allocator holds, read without a synchronisation."""
    out = []
    for seg in torch.cuda.memory_snapshot():
        addr = seg["address"]
        for b in seg["blocks"]:
            addr = b.get("address", addr)
            out.append((addr, b["size"], b["state"]))
            addr += b["size"]
    return out


MODELS = {
    # without the ln projection the trailing products read the encoder memory itself (the case that once broke)
    "no_ln": dict(V=5000, E=512, L=22, make=lambda V, E: build_no_ln(5)),
    "ln": dict(V=52, E=64, L=9, make=lambda V, E: build_model(V, E)),         # Cnn10's 512 channels -> E = 64 through ln
}


@pytest.mark.parametrize("persist", [True, False], ids=["default", "per_step"])
@pytest.mark.parametrize("which", sorted(MODELS))
def test_no_argument_of_decode_bwd_is_free_for_reuse_while_the_second_stream_is_behind(which, persist, monkeypatch):
    """See the module docstring.  There is no way to ask which path (persistent or per-step launches) a call took, so the
    test does not assert it; ``persist=False`` asks for the per-step launches."""
    cfg = MODELS[which]
    V, E, L, B, T = cfg["V"], cfg["E"], cfg["L"], 4, 160
    model = cfg["make"](V, E).train()
    assert hasattr(model, "ln") == (which == "ln")
    assert model.use_side_stream and model.defer_param_grads
    model.encoder.p_block = model.encoder.p_fc = 0.0
    model.decoder.dropoutlayer.p = 0.0
    feats, caps, fl, cl = O.synthetic_batch(B, T, V, L, seed=4, ragged=True)
    g = torch.Generator().manual_seed(3)
    noise = dict(eps_q=torch.randn(B, L - 1, E, generator=g), eps_p=torch.randn(L - 1, B, E, generator=g))
    feats_d = feats.cuda()

    def forward_loss():
        for p in model.parameters():
            p.grad = None
        model.noise = dict(noise)
        random.seed(9)
        torch.manual_seed(9)
        out = model(feats_d, fl.copy(), caps, cl, ss_ratio=1.0, dis_ratio=0)
        return out, hip_loss(out, caps, cl, V)[0]

    def grads():
        got = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
        assert got and all(bool(torch.isfinite(v).all()) for v in got.values())
        return got

    captured, answers = [], []
    real_call, real_defers = _lib.call, _lib.lib().acvae_decode_bwd_defers

    def call(name, *args):
        if name == "acvae_decode_bwd":
            captured.extend((t.data_ptr(), t.numel() * t.element_size()) for t in device_tensors(args))
        return real_call(name, *args)

    def defers(*args):
        answers.append(int(real_defers(*args)))
        return answers[-1]

    cycles = stall_cycles()
    with _lib.override(persist=persist):
        # one step first: the first launches of a process load code objects on the host, for longer than the stall lasts
        forward_loss()[1].backward()
        torch.cuda.synchronize()
        out, loss = forward_loss()
        side = model.streams.get("decode", torch.cuda.current_stream())
        stall_done = torch.cuda.Event()
        with torch.cuda.stream(side):
            torch.cuda._sleep(cycles)
            stall_done.record(side)
        monkeypatch.setattr(_lib, "call", call)
        monkeypatch.setattr(_lib.lib(), "acvae_decode_bwd_defers", defers)
        loss.backward()
        monkeypatch.undo()
        del out, loss
        states = block_states()                              # no synchronisation up to here
        still_stalled = not stall_done.query()
        torch.cuda.synchronize()
        assert answers == [1], f"acvae_decode_bwd_defers answered {answers}: nothing trails, the test exercises nothing"
        assert still_stalled, "stall too short: the second stream had passed it when the allocator's state was read"
        assert len(captured) > 40 and all(n > 0 for _, n in captured)
        # the allocator's three states: "active_allocated", freed and waiting for its recorded streams ("active_pending_free";
        # torch's documentation spells it "active_awaiting_free"), and "inactive" = free for reuse
        names = {s for _, _, s in states}
        assert "inactive" in names and all(s == "inactive" or s.startswith("active_") for s in names), names
        free_now, waiting = [], 0
        for ptr, n in captured:
            hit = [(a, sz, s) for a, sz, s in states if a <= ptr < a + sz]
            assert len(hit) == 1, f"argument at {ptr:#x} lies in {len(hit)} blocks of the allocator"
            if hit[0][2] == "inactive":
                free_now.append((hex(ptr), n))
            waiting += hit[0][2] not in ("inactive", "active_allocated")
        print(f"{len(captured)} tensor arguments: {waiting} freed and waiting for the second stream, {len(free_now)} free")
        assert not free_now, (f"{len(free_now)} of {len(captured)} tensor arguments of acvae_decode_bwd were free for reuse "
                              f"while its trailing work had not run: {free_now[:6]}")
        assert waiting > 0, "autograd has freed the upstream gradients: some block must be waiting for the second stream"
        two_streams = grads()
        model.use_side_stream = False
        out, loss = forward_loss()
        loss.backward()
        torch.cuda.synchronize()
        one_stream = grads()
    assert set(two_streams) == set(one_stream)
    bad = [n for n in one_stream if not torch.equal(two_streams[n], one_stream[n])]
    assert not bad, bad[:8]
