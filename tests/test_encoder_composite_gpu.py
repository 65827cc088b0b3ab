"""GPU: the fp32 encoders (acvae_encoder_fwd / acvae_encoder_bwd_hooked: Cnn10, Cnn14_16k, ResNet38) tensor by tensor against
float64, over every branch of the driver in csrc/encoder.hip - the fp32 twin of tests/test_bf16_oracle_gpu.py and the encoder's
twin of tests/test_decode_composite_gpu.py.

Every case of tests/encoder_ref.py CASES runs forward and backward of (audio_embeds * R).sum() on the HIP path (explicit
dropout masks in `train`, p_block = p_fc = 0 in `train_p0`, running statistics in `eval`), reads the ReLU decisions the
backward used (encoder.relu_masks()) and replays the reference in float64 and in fp32 under exactly those decisions.  A
decision may differ from the float64 replay's z > 0 only where |z| is below the flip zone the fp32-oracle tests use (1e-4
Cnn10, 1e-3 Cnn14_16k and ResNet38).  Then audio_embeds, audio_embeds_pooled, EVERY parameter gradient and in training the
batch's part of EVERY running statistic must satisfy

    rel_l2(HIP, float64) <= MARGIN max(alt, floor)      alt: rel_l2(fp32 reference, float64), floor: median alt over the gradients

(tests/encoder_ref.py ratio; tests/test_encoder_ref_cpu.py shows that this flags a BatchNorm epsilon of 2e-5, a missing Bessel
factor and a BatchNorm-backward mean over count - 1, all three of which pass the fixed 2e-4 / 5e-4 of the fp32-oracle tests).
In `eval` the running statistics and num_batches_tracked must be bit-unchanged.

Branches the cases take that no comparison reached before: the fp32 evaluation-mode backward (data-gradient filter images
built into scratch at backward time, bn_bwd with running statistics, the first conv's folded BatchNorm backward), training
without dropout, Cnn14_16k away from B = 4, T = 128 (odd heights in front of all five pools; T = 32: block 6 at H = 1,
W = 2), B = 33 clips of one output frame, the block_done callback outside a process group (`hooked`: the sequence is every
block from the deepest down, then "encoder", and the gradients are bit-equal to the unhooked run's) and, in one child
process with ACVAE_CONV_WINO=0 (read once per process), the implicit-GEMM route of three of the cases (`igemm`).

MARGIN (tests/encoder_ref.py): 8.0 Cnn10, 12.0 Cnn14_16k, 8.0 ResNet38.  The comparison started from
tests/test_bf16_oracle_gpu.py's 4.0 / 8.0 / 8.0.  Worst measured ratio on the MI355X per family (test_zz_worst_ratio_per_arch
prints the table):
    Cnn10       5.03  conv_block2.bn2.bias, B=3 T=47 train, implicit GEMM (its Winograd twin: 3.96)
                4.14  conv_block1.bn2.bias, B=2 T=96 eval, the worst on the default route (its implicit-GEMM twin: 2.71)
    Cnn14_16k   8.06  conv_block2.bn2.weight, B=8 T=32 train (5.7e-5 from float64 against a yardstick of 7.1e-6)
                7.50  conv_block5.bn1.bias, B=4 T=128 eval (1.0e-5 against 1.2e-6)
    ResNet38    5.51  resnet.layer3.5.bn1.bias, B=2 T=64 eval (2.2e-6 against 3.9e-7)
Six tensors in three cases were over 4.0 / 8.0 and none was an error: MARGIN's comment in tests/encoder_ref.py gives the
rounding cause (one k-ordered MFMA chain per convolution output against the CPU library's interleaved partial sums) and what
was measured for it - the distances stay under the kernel tests' 1e-5 per kernel, and the two convolution routes of one case
err independently of each other.  No ReLU decision differed at |z| above 1.5e-5; the hooked run was bit-equal.  No case found
a defect in the driver."""
import json
import os
import subprocess
import sys

import pytest
import torch

import encoder_ref as E
from acvae_amd.encoder import Cnn10, Cnn14_16k, ResNet38

pytestmark = pytest.mark.gpu
IGEMM_CHILD = os.environ.get("ACVAE_CONV_WINO") == "0"
TAG = "ENCODER-COMPOSITE "
WORST = {}          # arch -> (ratio, tensor, case)
_child = {}


@pytest.fixture(autouse=True)
def threads():
    torch.set_num_threads(min(16, os.cpu_count() or 1))


def make_encoder(case, d):
    enc = {"Cnn10": Cnn10, "Cnn14_16k": Cnn14_16k, "ResNet38": ResNet38}[case.arch](64, E.WIDTH[case.arch])
    enc.load_state_dict({k: v.clone() for k, v in d["state"].items()})
    return enc.cuda()


def run_hip(case, cb=None):
    """The case on the HIP path -> ({tensor: value on the host}, its ReLU decisions, the module)."""
    d = E.inputs(case)
    enc = make_encoder(case, d)
    enc.train(case.training)
    enc.keep_saved = True
    if case.mode == "train":
        enc.dropout_masks = [m.clone() for m in d["masks"]]
    elif case.mode == "train_p0":
        enc.p_block = enc.p_fc = 0.0
    enc._grad_ready_cb = cb
    before = {k: v.detach().clone() for k, v in enc.state_dict().items()}
    out = enc(d["feats"].cuda(), list(d["lens"]))
    relu = [m.cpu() for m in enc.relu_masks()]
    (out["audio_embeds"] * d["R"].cuda()).sum().backward()
    torch.cuda.synchronize()
    assert out["audio_embeds_lens"].tolist() == [case.T // E.DIV[case.arch]] * case.B
    got = {"audio_embeds": out["audio_embeds"].detach().cpu(), "audio_embeds_pooled": out["audio_embeds_pooled"].detach().cpu()}
    for k, p in enc.named_parameters():
        if k.startswith(E.HEAD[case.arch] + "."):
            assert p.grad is None, k
        else:
            got[k] = p.grad.detach().cpu()
    for k, v in enc.state_dict().items():
        if k.endswith(("running_mean", "running_var")):
            if case.training:
                got[k] = v.detach().cpu().double() - 0.9 * before[k].cpu().double()
            else:
                assert torch.equal(v, before[k]), f"{case.name}: evaluation mode wrote {k}"
        elif k.endswith("num_batches_tracked"):
            assert int(v) == int(before[k]) + int(case.training), (case.name, k)
    return got, relu, enc


def judge(case, got, relu):
    """-> dict(name, arch, worst, tensor, flips, zmax, failures)"""
    y, zs = E.yardstick_z(case, relu)
    assert len(zs) == len(relu)
    flips, zmax = 0, 0.0
    for m, z in zip(relu, zs):
        dif = m != (z > 0)
        if bool(dif.any()):
            flips += int(dif.sum())
            zmax = max(zmax, float(z[dif].abs().max()))
    failures = []
    if zmax >= E.FLIP_ZONE[case.arch]:
        failures.append(f"{flips} ReLU decisions differ from the float64 replay, one at |z| = {zmax:.2e}")
    for k, v in got.items():
        if not bool(torch.isfinite(v).all()):
            failures.append(f"{k} is not finite")
    ratios = E.ratio(got, case, y=y)
    floor, margin = E.floor_of(y), E.MARGIN[case.arch]
    worst = max(ratios, key=ratios.get)
    for k in sorted(ratios, key=ratios.get, reverse=True):
        if not ratios[k] <= margin:
            failures.append(f"{k}: {E.rel_l2(got[k], y[k][0]):.2e} from float64, {ratios[k]:.1f} x max(alt {y[k][1]:.2e}, "
                            f"floor {floor:.2e})")
    print(f"\n{case.name}: worst ratio {ratios[worst]:.2f} ({worst}: {E.rel_l2(got[worst], y[worst][0]):.2e}, alt "
          f"{y[worst][1]:.2e}, floor {floor:.2e}) over {len(ratios)} tensors; {flips} decisions differ (max |z| {zmax:.1e})")
    return dict(name=case.name, arch=case.arch, worst=ratios[worst], tensor=worst, flips=flips, zmax=zmax, failures=failures)


def note(res):
    if res["worst"] > WORST.get(res["arch"], (-1.0, "", ""))[0]:
        WORST[res["arch"]] = (res["worst"], res["tensor"], res["name"])


def igemm_child():
    """The `igemm` cases of this file in ONE child process with ACVAE_CONV_WINO=0 -> {case name: judge()'s dict}."""
    if not _child:
        torch.cuda.synchronize()            # (a device this process has faulted gets no further process)
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-s", "-p", "no:cacheprovider",
                            "-k", "igemm"], env=dict(os.environ, ACVAE_CONV_WINO="0"), capture_output=True, text=True,
                           timeout=600)
        _child["tail"] = r.stdout[-3000:] + r.stderr[-1000:]
        _child["res"] = {}
        for line in r.stdout.splitlines():
            if TAG in line:
                res = json.loads(line[line.index(TAG) + len(TAG):])
                _child["res"][res["name"]] = res
    return _child["res"], _child["tail"]


@pytest.mark.parametrize("case", E.CASES, ids=E.CASE_IDS)
def test_encoder_composite(case):
    if case.route == "igemm" and not IGEMM_CHILD:
        results, tail = igemm_child()
        assert case.name in results, tail
        res = results[case.name]
        print(f"\n{case.name} (child process, ACVAE_CONV_WINO=0): worst ratio {res['worst']:.2f} ({res['tensor']}); "
              f"{res['flips']} decisions differ (max |z| {res['zmax']:.1e})")
    else:
        got, relu, enc = run_hip(case)
        if case.hooked:
            seen = []
            got_h, relu_h, _ = run_hip(case, seen.append)
            nb = enc.N_BLOCKS
            assert seen[0] == ("encoder_block", enc._deep_block()[1]), seen
            assert seen == [("encoder_block", b) for b in range(nb, 0, -1)] + ["encoder"], seen
            assert all(torch.equal(a, b) for a, b in zip(relu, relu_h))
            assert set(got) == set(got_h)
            for k in got:
                assert torch.equal(got[k], got_h[k]), f"{case.name}: {k} differs in bits from the unhooked run"
            got, relu = got_h, relu_h
        res = judge(case, got, relu)
        if IGEMM_CHILD:
            print("\n" + TAG + json.dumps(res))
    note(res)
    assert not res["failures"], f"{case.name}: " + "; ".join(res["failures"])


def test_zz_worst_ratio_per_arch():
    """Prints the worst measured ratio per family (the figures of the module docstring and DESIGN.md); runs last, over whatever
    cases ran before it."""
    for arch, (r, tensor, name) in sorted(WORST.items()):
        print(f"\n{arch}: worst ratio {r:.2f} of margin {E.MARGIN[arch]} ({tensor} in {name})")
    assert all(r <= E.MARGIN[arch] for arch, (r, _, _) in WORST.items())
