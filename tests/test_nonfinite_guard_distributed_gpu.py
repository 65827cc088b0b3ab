"""GPU: the non-finite guard under data parallelism.  Two ranks on GPU 0 over gloo, a different shard per rank and step:

  1. a good step, then a step in which rank 1 ALONE gets a batch with a NaN feature: both ranks skip (the exchanged
     gradients carry the NaN to rank 0, the all-reduced witness flag the rest), and both hold the parameters, the optimiser
     state and the BatchNorm statistics of before, bit for bit and equal to each other;
  2. the next good step leaves both ranks bit-identical again, and agrees with ONE process that resumes from rank 0's
     checkpoint and takes the two shards as one accumulation window, within the bound
     tests/test_accumulate_distributed_gpu.py holds that pair to (rtol 1e-5 / atol 1e-6).
"""
import os
import queue
import time
import traceback

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_accumulate_distributed_gpu import V, _free_port, _model, _shard, _step

pytestmark = pytest.mark.gpu
DEADLINE = 300.0


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().copy()


def _state(ts):
    torch.cuda.synchronize()
    return {"flat_p": _bits(ts.flat_p), "exp_avg": _bits(ts.exp_avg), "exp_avg_sq": _bits(ts.exp_avg_sq),
            "flat_buf": _bits(ts.flat_buf)}


def _body(rank, world):
    from acvae_amd.trainer import TrainStep
    model = _model()
    ts = TrainStep(model, V, nonfinite="skip")
    assert ts.world == world
    p0 = _step(ts, model, _shard(rank, 0))
    oks = [int(p0["update_ok"].item())]            # (a view of the record: read before the next decision overwrites it)
    ts.sync_buffers()
    before = _state(ts)
    shard = list(_shard(rank, 1))
    if rank == 1:
        shard[0] = shard[0].clone()
        shard[0][1, 7, 3] = float("nan")
    p1 = _step(ts, model, tuple(shard))
    ts.sync_buffers()
    after_bad = _state(ts)
    oks.append(int(p1["update_ok"].item()))
    counts_bad = ts.guard_counts()
    local_loss_finite = bool(torch.isfinite(p1["loss"]).all())
    single = None
    if rank == 0:                                   # one process resumes from this rank's checkpoint
        model1 = _model()
        ts1 = TrainStep(model1, V, data_parallel=False, accum_steps=2, nonfinite="skip")
        model1.load_state_dict({k: v.clone() for k, v in model.state_dict().items()})
        ts1.load_optimizer_state_dict(ts.optimizer_state_dict())
        assert ts1.world == 1 and np.array_equal(_bits(ts1.flat_p), before["flat_p"])
        for r in range(world):
            q = _step(ts1, model1, _shard(r, 2))
        assert q["applied"] is True and int(q["update_ok"].item()) == 1
        single = ts1.flat_p.cpu().numpy().copy()
    p2 = _step(ts, model, _shard(rank, 2))
    ts.sync_buffers()
    oks.append(int(p2["update_ok"].item()))
    ts.synchronize()
    return dict(before=before, after_bad=after_bad, after=_state(ts), oks=oks, counts_bad=counts_bad,
                counts=ts.guard_counts(), loss_finite=local_loss_finite, single=single,
                flat=ts.flat_p.cpu().numpy().copy(), start=before["flat_p"].view(np.float32).copy())


def _worker(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        res = _body(rank, world)
    except BaseException:
        q.put((rank, None, traceback.format_exc()))
        raise
    q.put((rank, res, None))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_one_gpu_gloo_skip_together():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
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
    # 1. both ranks skip the step in which rank 1 alone had the bad batch; nothing moved, on either rank
    assert a["oks"] == b["oks"] == [1, 0, 1]
    assert a["loss_finite"]                          # rank 0's own batch was fine: it skips on rank 1's account
    print(f"rank 1's loss on the bad batch finite: {b['loss_finite']}")
    want = {"applied": 1, "skipped": 1, "streak": 1}
    assert a["counts_bad"] == b["counts_bad"] == want
    for k in a["before"]:
        assert np.array_equal(a["after_bad"][k], a["before"][k]), f"rank 0: {k} moved on the skipped step"
        assert np.array_equal(b["after_bad"][k], b["before"][k]), f"rank 1: {k} moved on the skipped step"
        # (the buffers are rank 0's on both ranks: broadcast_buffers)
        assert np.array_equal(a["after_bad"][k], b["after_bad"][k]), f"{k} differs between the ranks"
    # 2. the next step: the ranks agree bit for bit, and with one process over the same two shards
    assert a["counts"] == b["counts"] == {"applied": 2, "skipped": 1, "streak": 0}
    for k in a["after"]:
        assert np.array_equal(a["after"][k], b["after"][k]), f"{k} differs between the ranks after the next step"
    assert not np.array_equal(a["after"]["flat_p"], a["before"]["flat_p"])
    got, ref = a["flat"].astype(np.float64), a["single"].astype(np.float64)
    assert np.isfinite(got).all() and np.isfinite(ref).all()
    moved = np.abs(ref - a["start"]).max()
    assert moved > 1e-4, moved
    err = np.abs(got - ref)
    ok = err <= 1e-6 + 1e-5 * np.abs(ref)
    print(f"gloo guard: max err {err.max():.3e}, {int((~ok).sum())}/{ok.size} out of tolerance, moved {moved:.3e}, "
          f"bit-equal {np.array_equal(a['flat'], a['single'])}")
    assert ok.all(), f"max err {err.max():.3e}, {int((~ok).sum())}/{ok.size} out of tolerance"
