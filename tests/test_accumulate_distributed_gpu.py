"""GPU: gradient accumulation under data parallelism.  Two ranks (both on GPU 0 over gloo; one GPU each over RCCL where two
are visible), accum_steps=2, a different shard per rank and per micro-step:

  1. the first micro-step issues no collective (exchange.issued == []) and leaves the parameters alone;
  2. the second all-reduces flat_acc once, in pieces of at most max_chunk elements, the same (bucket, piece) sequence on
     both ranks;
  3. after the window both ranks hold bit-identical parameters;
  4. they agree with ONE process that accumulates the four shards with accum_steps=4 (the mean of the same four gradients,
     summed in another order) within the bound the optimiser tests hold their torch twins to, rtol 1e-5 / atol 1e-6.
"""
import os
import queue
import random
import socket
import time
import traceback

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
V, E, L, NB, T = 60, 64, 8, 3, 64
MAX_CHUNK = 1 << 20
OPT = {}                                # TrainStep's optimiser arguments (the default: Adam)
DEADLINE = 300.0                        # for the whole exchange with the children; a rank that fails ends the wait at once


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _model():
    from acvae_amd.decoder import VAERNNBahdanauAttnDecoder
    from acvae_amd.encoder import Cnn10
    from acvae_amd.vae_model import Hybrid_VAEModel
    torch.manual_seed(5)
    dec = VAERNNBahdanauAttnDecoder(vocab_size=V, enc_mem_size=E, embed_size=E, hidden_size=E, attn_size=E)
    m = Hybrid_VAEModel(Cnn10(64, 512), dec, posterior_model="PosteriorRNN_hybrid", posterior_args={"hidden_size": E},
                        prior_model="PriorRNN", prior_args={"hidden_size": E}).cuda().train()
    m.encoder.p_block = m.encoder.p_fc = 0.0
    return m


def _shard(rank, step):
    g = torch.Generator().manual_seed(10 + rank + 100 * step)
    feats = torch.randn(NB, T, 64, generator=g)
    caps = torch.zeros(NB, L); caps[:, 0] = 1; caps[:, -1] = 2
    caps[:, 1:-1] = torch.randint(4, V, (NB, L - 2), generator=g).float()
    eps_q = torch.randn(NB, L - 1, E, generator=g)
    eps_p = torch.randn(L - 1, NB, E, generator=g)
    return feats, caps, np.full(NB, T), np.full(NB, L), eps_q, eps_p


def _step(ts, model, shard):
    feats, caps, fl, cl, eps_q, eps_p = shard
    model.noise = dict(eps_q=eps_q, eps_p=eps_p)
    random.seed(1)
    parts = ts.step(feats.cuda(), fl.copy(), caps, cl, 1.0, 0, 0.5)
    torch.cuda.synchronize()
    return parts


def _body(rank, world, backend, opt):
    from acvae_amd.trainer import TrainStep
    model = _model()
    ts = TrainStep(model, V, accum_steps=2, **opt)
    ts.exchange.max_chunk = MAX_CHUNK
    assert ts.world == world and ts.exchange.flat is ts.flat_acc
    start = ts.flat_p.clone()
    p1 = _step(ts, model, _shard(rank, 0))
    issued1 = list(ts.exchange.issued)
    assert p1["applied"] is False and "grad_norm" not in p1
    assert torch.equal(ts.flat_p, start) and ts.step_count == 0 and ts.micro_count == 1
    assert ts._buf_work is not None                 # the BatchNorm-buffer broadcast stays behind every micro-step
    p2 = _step(ts, model, _shard(rank, 1))
    issued2 = list(ts.exchange.issued)
    assert p2["applied"] is True and ts.step_count == 1 and ts.micro_count == 0
    assert not torch.equal(ts.flat_p, start)
    pieces = sum(-(-(b - a) // MAX_CHUNK) for a, b in ts.exchange.slices)
    flat = ts.flat_p.cpu().numpy().copy()
    single = None
    if rank == 0:                                   # one process, the four shards as four micro-steps
        model4 = _model()
        ts4 = TrainStep(model4, V, data_parallel=False, accum_steps=4, **opt)
        assert ts4.world == 1 and torch.equal(ts4.flat_p, start)
        for step in range(2):
            for r in range(world):
                p4 = _step(ts4, model4, _shard(r, step))
        assert p4["applied"] is True and ts4.exchange.issued == []
        single = ts4.flat_p.cpu().numpy().copy()
    return dict(issued1=issued1, issued2=issued2, pieces=pieces, flat=flat, single=single, start=start.cpu().numpy(),
                norm=float(p2["grad_norm"]), loss=(float(p1["loss"]), float(p2["loss"])))


def _worker(rank, world, port, backend, q, opt):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        torch.cuda.set_device(rank if backend == "nccl" else 0)
        dist.init_process_group(backend, rank=rank, world_size=world)
        res = _body(rank, world, backend, opt)
    except BaseException:
        q.put((rank, None, traceback.format_exc()))
        raise
    q.put((rank, res, None))
    dist.barrier()
    dist.destroy_process_group()


def _run(backend, opt=OPT):
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, world, port, backend, q, opt)) for r in range(world)]
    for p in ps:
        p.start()
    res, failed = {}, None
    end = time.monotonic() + DEADLINE
    try:
        while len(res) < world and failed is None:
            try:
                rank, r, err = q.get(timeout=1.0)
            except queue.Empty:
                dead = [p for p in ps if p.exitcode not in (None, 0)]
                if dead:
                    failed = f"a rank ended with exit code {dead[0].exitcode} before it reported"
                elif time.monotonic() > end:
                    failed = "the ranks did not report in time"
                continue
            if err is not None:
                failed = f"rank {rank} failed:\n{err}"
            res[rank] = r
    finally:
        if failed is not None:
            for p in ps:
                p.terminate()
        for p in ps:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
                p.join(timeout=10)
    assert failed is None, failed
    assert all(p.exitcode == 0 for p in ps), [p.exitcode for p in ps]
    a, b = res[0], res[1]
    # 1. no collective in the first micro-step
    assert a["issued1"] == [] and b["issued1"] == []
    # 2. one exchange of flat_acc, bucket by bucket in pieces of at most MAX_CHUNK, the same on both ranks
    assert a["issued2"] == b["issued2"] and len(a["issued2"]) == a["pieces"] > 4, (a["issued2"], a["pieces"])
    assert [bk for bk, _ in a["issued2"]] == sorted(bk for bk, _ in a["issued2"]) and {bk for bk, _ in a["issued2"]} == {0, 1, 2, 3}
    # 3. bit-identical parameters (the shards, hence the local losses, differ)
    assert np.array_equal(a["flat"], b["flat"]) and a["norm"] == b["norm"] and a["loss"] != b["loss"]
    # 4. against one process accumulating the four shards
    got, ref = a["flat"].astype(np.float64), a["single"].astype(np.float64)
    moved = np.abs(ref - a["start"]).max()
    assert moved > 1e-4, moved
    err = np.abs(got - ref)
    ok = err <= 1e-6 + 1e-5 * np.abs(ref)
    print(f"{backend} {opt}: max err {err.max():.3e}, {int((~ok).sum())}/{ok.size} out of tolerance, moved {moved:.3e}")
    assert ok.all(), f"max err {err.max():.3e}, {int((~ok).sum())}/{ok.size} out of tolerance"


def test_two_ranks_one_gpu_gloo_accumulate():
    _run("gloo")


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="RCCL needs one GPU per rank: two GPUs")
def test_two_ranks_rccl_accumulate():
    _run("nccl")
