"""One sha256 per output tensor of every inference search route, through the public API only
(``model(feats, feat_lens, method=...)`` and ``Ensemble(models)(feats, feat_lens, ...)``), at small shapes under fixed
seeds: N = 2 clips of 64 frames, max_length 6, a vocabulary of 60.  Two trees whose searches compute the same bits print
the same lines, so a change that is meant to leave every result alone is checked by running this file from both trees
(one process each, on the same machine) and comparing the outputs.

  python tools/search_digest.py            one line per tensor: <route> <key> <dtype> <shape> <sha256>
                                           (a lengths tensor is small: its values follow, to show what the route met)
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

N, FRAMES, T, V = 2, 64, 6, 60
CONSTRAIN = dict(repetition_penalty=1.2, no_repeat_ngram_size=2, min_length=2, suppress_tokens=[5, 7])
BEAM_MODES = {"plain": {}, "constrained": CONSTRAIN, "finishing": dict(finish_on_end=True, length_penalty=0.7, nbest=3)}


def member(seed, E, H, A, end_bump):
    from acvae_amd.decoder import VAERNNBahdanauAttnDecoder
    from acvae_amd.encoder import Cnn10
    from acvae_amd.vae_model import Hybrid_VAEModel
    torch.manual_seed(seed)
    dec = VAERNNBahdanauAttnDecoder(vocab_size=V, enc_mem_size=E, embed_size=E, hidden_size=H, dropout=0.0, num_layers=1,
                                    rnn_type="GRU", attn_size=A)
    model = Hybrid_VAEModel(Cnn10(64, 512), dec, posterior_model="PosteriorRNN_hybrid", posterior_args={"hidden_size": E},
                            prior_model="PriorRNN", prior_args={"hidden_size": E})
    with torch.no_grad():                                 # spread the word scores so that the routes pick different words,
        model.decoder.classifier.weight.mul_(8.0)         # and let <end> win now and then: hypotheses of unequal lengths
        model.decoder.classifier.bias[int(model.end_idx)] += end_bump
    return model.cuda().eval()


def digest(route, out):
    for key in sorted(out):
        value = out[key]
        if not isinstance(value, torch.Tensor):
            continue
        a = value.detach().cpu().contiguous().numpy()
        shown = " " + str(a.tolist()).replace(" ", "") if "lengths" in key else ""
        print(route, key, a.dtype, "x".join(map(str, a.shape)), hashlib.sha256(a.tobytes()).hexdigest() + shown, flush=True)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("search_digest.py runs the searches on the GPU: none found")
    from acvae_amd.ensemble import Ensemble
    one = member(11, 64, 64, 64, 6.0)
    pair = [member(12, 64, 96, 160, 4.0), member(13, 128, 64, 64, 4.0)]        # unequal widths, H != E within each
    feats = torch.randn(N, FRAMES, 64, generator=torch.Generator().manual_seed(3)).cuda()
    lens = np.array([FRAMES, FRAMES - 16])

    def run(route, model, seed, **kw):
        torch.manual_seed(seed)
        with torch.no_grad():
            digest(route, model(feats, lens.copy(), **kw))

    run("ensemble2.greedy", Ensemble(pair), 20, method="greedy", max_length=T)
    for mode, kw in BEAM_MODES.items():
        run(f"one.beam3.{mode}", one, 21, method="beam", beam_size=3, max_length=T, **kw)
        run(f"ensemble2.beam3.{mode}", Ensemble(pair), 22, method="beam", beam_size=3, max_length=T, **kw)
    run("one.dbs.G2b2", one, 23, method="dbs", beam_size=4, group_size=2, max_length=T)
    run("one.dbs.G3T2", one, 24, method="dbs", beam_size=3, group_size=3, max_length=2)
    run("ensemble2.dbs.G2b2", Ensemble(pair), 25, method="dbs", beam_size=4, group_size=2, max_length=T)
    run("one.dbs.host", one, 26, method="dbs", beam_size=4, group_size=2, max_length=T, dbs_impl="host")
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
