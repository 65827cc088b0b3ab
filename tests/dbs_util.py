"""Yardsticks of the one-call diverse beam search (acvae_dbs_search / acvae_ensemble_dbs_search, include/acvae_hip.h).

Three things, all bit-exact (no tolerance anywhere):

1. A numpy twin of the device bookkeeping on the tables the library keeps, int32 [G][T][R] (row r = n * bdash + b):
   `advance` (record and retire behind a top-k), `dense_counts` (the penalty's count vector, read from the earlier groups'
   tables by walking the parents), `finish` (rank the records by the fp64 key, trace the parents).
2. `naive_search`: the same search the way the reference writes it, with lists of hypotheses that are re-gathered and
   concatenated every step, on given score tables.  `table_search` runs the twin on the same tables; the two must agree.
3. `host_loop`: Hybrid_VAEModel.diverse_beam_search_host generalised to M members, over the step API plus the
   acvae_ensemble_mix, acvae_dbs_scores and acvae_topk_flat_batched ops (GPU only).

The schedule: pairs (t, g), t = 0 .. T + G - 2, g = 0 .. G - 1 with 0 <= lt = t - g <= T - 1, in that order."""
import numpy as np

NONE = np.float32(np.nan)           # "no record" in the record table


def schedule(T, G):
    return [(t, g) for t in range(T + G - 1) for g in range(G) if 0 <= t - g <= T - 1]


def topk_flat(x, k):
    """Sorted descending, ties to the lower index: acvae_topk_flat_batched's order.  -> (values, flat indices)."""
    order = np.argsort(-x.astype(np.float64), kind="stable")[:k]
    return x[order], order


# ------------------------------------------------------------------------------------------------ the twin
def advance(c, parent, word, end_idx, last):
    """One acvae_dbs_advance: c f32 [R], parent / word int64 [R] -> (parent i32, word i32, rec f32, c after)."""
    c = np.asarray(c, np.float32)
    ends = (np.asarray(word) == end_idx) | bool(last)
    rec = np.where(ends, c, NONE).astype(np.float32)
    after = np.where(ends, c - np.float32(1000.0), c).astype(np.float32)
    return np.asarray(parent).astype(np.int32), np.asarray(word).astype(np.int32), rec, after


def column_words(par_tab, word_tab, e, le, lt, rows):
    """The words the rows `rows` of group e, as they stand after local step le, hold at column lt."""
    R = par_tab.shape[2]
    r = np.array(rows, dtype=np.int64)
    for s in range(le, lt, -1):
        r = np.clip(par_tab[e, s, r].astype(np.int64), 0, R - 1)
    return word_tab[e, lt, r]


def dense_counts(par_tab, word_tab, N, bdash, T, V, g, lt):
    """count[n, c] f32 [N, V]: the beams of the groups e < g of clip n whose current history holds c at column lt."""
    counts = np.zeros((N, V), np.float32)
    for n in range(N):
        for e in range(g):
            le = min(lt + g - e, T - 1)
            w = column_words(par_tab, word_tab, e, le, lt, range(n * bdash, (n + 1) * bdash))
            w = w[(w >= 0) & (w < V)]
            np.add.at(counts[n], w, np.float32(1.0))
    return counts


def finish(par_tab, word_tab, rec, N, G, bdash, T, group_nbest, end_idx):
    """acvae_dbs_finish: -> (seqs i64 [N, rows, T], scores f64 [N, rows], lengths i32 [N, rows])."""
    keep = bdash if group_nbest else 1
    R = N * bdash
    seqs = np.full((N, G * keep, T), end_idx, np.int64)
    scores = np.full((N, G * keep), -np.inf, np.float64)
    lengths = np.zeros((N, G * keep), np.int32)
    for n in range(N):
        for g in range(G):
            cands = []
            for lt in range(T):
                for b in range(bdash):
                    c = rec[g, lt, n * bdash + b]
                    if c == c:
                        cands.append((np.float64(c) / np.float64(lt + 1), lt * bdash + b))
            taken = []
            for q in range(keep):
                best = None
                for v, i in cands:
                    if i in taken:
                        continue
                    if best is None or v > best[0] or (v == best[0] and i < best[1]):
                        best = (v, i)
                if best is None:
                    continue
                taken.append(best[1])
                lt0, b = divmod(best[1], bdash)
                o = g * keep + q
                scores[n, o], lengths[n, o] = best[0], lt0 + 1
                r = n * bdash + b
                for t in range(lt0, -1, -1):
                    seqs[n, o, t] = word_tab[g, t, r]
                    r = min(max(int(par_tab[g, t, r]), 0), R - 1)
    return seqs, scores, lengths


def _scores(logp, prev, counts, lam):
    """The penalty and the running score on given per-word log-probabilities: v -= count * lambda, then prev + v (fp32)."""
    v = logp.astype(np.float32).copy()
    if counts is not None:
        v = (v - counts.astype(np.float32) * np.float32(lam)).astype(np.float32)
    return (prev.astype(np.float32)[:, None] + v).astype(np.float32)


def table_search(logp, N, G, bdash, T, V, lam, group_nbest, end_idx):
    """The search on given tables logp[g][lt] f32 [R, V] (a step's log-probabilities do not depend on the past here),
    through the twin: tables, `dense_counts`, `advance`, `finish`."""
    R = N * bdash
    par_tab = np.zeros((G, T, R), np.int32)
    word_tab = np.zeros((G, T, R), np.int32)
    rec = np.full((G, T, R), NONE, np.float32)
    running = np.zeros((G, R), np.float32)
    for t, g in schedule(T, G):
        lt = t - g
        counts = dense_counts(par_tab, word_tab, N, bdash, T, V, g, lt) if g > 0 else None
        sc = _scores(logp[g][lt], running[g], None if counts is None else np.repeat(counts, bdash, axis=0), lam)
        c, parent, word = np.zeros(R, np.float32), np.zeros(R, np.int64), np.zeros(R, np.int64)
        for n in range(N):
            flat = sc[n * bdash:(n + 1) * bdash].reshape(-1)
            vals, idx = topk_flat(flat[:V] if lt == 0 else flat, bdash)
            c[n * bdash:(n + 1) * bdash] = vals
            parent[n * bdash:(n + 1) * bdash] = n * bdash + idx // V
            word[n * bdash:(n + 1) * bdash] = idx % V
        par_tab[g, lt], word_tab[g, lt], rec[g, lt], running[g] = advance(c, parent, word, end_idx, lt == T - 1)
    return finish(par_tab, word_tab, rec, N, G, bdash, T, group_nbest, end_idx), (par_tab, word_tab, rec)


# ------------------------------------------------------------------------------------------------ the naive search
def naive_search(logp, N, G, bdash, T, V, lam, group_nbest, end_idx):
    """The same search as the reference writes it (models/word_model.py:297-394): per clip and group a list of hypotheses
    (word lists) that is re-gathered by the parents and extended every step, a list of finished hypotheses with
    score = float(c) / length, Python's stable sort at the end.  No tables, no parents kept."""
    rows = G * bdash if group_nbest else G
    seqs = np.full((N, rows, T), end_idx, np.int64)
    scores = np.zeros((N, rows), np.float64)
    lengths = np.zeros((N, rows), np.int32)
    for n in range(N):
        hyps = [[[] for _ in range(bdash)] for _ in range(G)]
        running = [np.zeros(bdash, np.float32) for _ in range(G)]
        done = [[] for _ in range(G)]
        for t, g in schedule(T, G):
            lt = t - g
            counts = None
            if g > 0:
                counts = np.zeros(V, np.float32)
                for e in range(g):
                    for h in hyps[e]:
                        counts[h[lt]] += np.float32(1.0)
            sc = _scores(logp[g][lt][n * bdash:(n + 1) * bdash], running[g], None if counts is None else counts[None, :], lam)
            flat = sc.reshape(-1)
            vals, idx = topk_flat(flat[:V] if lt == 0 else flat, bdash)
            hyps[g] = [list(hyps[g][int(i) // V]) + [int(i) % V] for i in idx]
            vals = vals.copy()
            for b in range(bdash):
                if hyps[g][b][lt] == end_idx or lt == T - 1:
                    done[g].append({"seq": list(hyps[g][b]), "score": float(vals[b]) / (lt + 1)})
                    vals[b] -= np.float32(1000)
            running[g] = vals
        ranked = [sorted(d, key=lambda x: -x["score"])[:bdash] for d in done]
        chosen = sum(ranked, []) if group_nbest else [d[0] for d in ranked]
        for r, h in enumerate(chosen):
            seqs[n, r, :len(h["seq"])] = h["seq"]
            scores[n, r], lengths[n, r] = h["score"], len(h["seq"])
    return seqs, scores, lengths


# ------------------------------------------------------------------------------------------------ the host loop, M members
def host_loop(models, feats, feat_lens, max_length, beam_size, group_size, diversity_lambda=0.5, temperature=1.0,
              group_nbest=True):
    """Hybrid_VAEModel.diverse_beam_search_host over M members (GPU): every member steps on the shared word through its
    step modules; with M > 1 one acvae_ensemble_mix launch (prev = NULL) forms the rows acvae_dbs_scores is fed in the
    logits' place; counts from the host lists, acvae_topk_flat_batched, three read-backs per step.  Member m's noise is
    drawn with the calls its own search makes, members in order.  -> (seqs, scores, lengths) as numpy arrays."""
    import torch
    from acvae_amd import _lib
    m0 = models[0]
    G, T = group_size, max_length
    bdash = beam_size // group_size
    V, end_idx = m0.vocab_size, int(m0.end_idx)
    steps = schedule(T, G)
    st = _lib.current_stream
    members = []
    with torch.no_grad():
        for model in models:
            model.eval()
            model._forward_token = getattr(model, "_forward_token", 0) + 1
            enc = model.encoder(feats, np.asarray(feat_lens).copy())
            mem_all = model._projected_memory(enc)
            N, S, E = mem_all.shape
            dev = mem_all.device
            eps = torch.empty(N, len(steps), bdash, E)
            for i in range(N):
                for k in range(len(steps)):
                    torch.randn(bdash, E, out=eps[i, k])
            members.append(dict(model=model, mem=mem_all.repeat_interleave(bdash, dim=0).contiguous(),
                                lens=torch.as_tensor(enc["audio_embeds_lens"]).to(torch.long).repeat_interleave(bdash),
                                eps=eps.to(dev), E=E, carry=[None] * G))
        R = N * bdash
        scores = torch.empty(R, V, device=dev)
        mixed = torch.empty(R, V, device=dev)
        vals = torch.empty(R, device=dev)
        idx, prev_d, nxt_d = (torch.empty(R, dtype=torch.long, device=dev) for _ in range(3))
        seq = [[np.zeros((bdash, 0), np.int64) for _ in range(G)] for _ in range(N)]
        score = [np.zeros((N, bdash), np.float32) for _ in range(G)]
        done = [[[] for _ in range(G)] for _ in range(N)]
        words, parents = [None] * G, [None] * G
        base = (np.arange(N) * bdash)[:, None]
        ld = np.full(len(models), V, dtype=np.int64)
        for k, (t, g) in enumerate(steps):
            lt = t - g
            logits = []
            for mb in members:
                model, E = mb["model"], mb["E"]
                if lt == 0:
                    w = torch.full((R,), int(model.start_idx), dtype=torch.long, device=dev)
                    state = model.decoder.init_hidden(R).to(dev)
                    hid = model.pnet.init_hidden(R, dev)
                    last_z = torch.zeros(R, E, device=dev)
                else:
                    state0, hid0, z0 = mb["carry"][g]
                    w, parent = words[g], parents[g]
                    state = state0[:, parent].contiguous()
                    hid = (hid0[0][:, parent].contiguous(), hid0[1][:, parent].contiguous())
                    last_z = z0[parent].contiguous()
                pn = model.pnet(w.unsqueeze(1), mb["mem"], hid, last_z, mb["lens"], eps=mb["eps"][:, k].reshape(R, E))
                dn = model.decoder(word=w.unsqueeze(1), state=state, enc_mem=mb["mem"], enc_mem_lens=mb["lens"], z=pn["z"])
                logits.append(dn["logits"].squeeze(1).contiguous())
                mb["carry"][g] = (dn["state"], pn["hiddens_state"], pn["z"])
            x = logits[0]
            if len(models) > 1:
                _lib.call("acvae_ensemble_mix", _lib.ptr_table(logits), ld.ctypes.data, len(models), None, mixed, V, None, None,
                          0, R, V, st())
                x = mixed
            counts = None
            if g > 0:
                c = np.zeros((N, V), np.float32)
                for i in range(N):
                    for earlier in range(g):
                        np.add.at(c[i], seq[i][earlier][:, lt], 1.0)
                counts = torch.from_numpy(c).to(dev)
            _lib.call("acvae_dbs_scores", x, V, float(temperature), counts, float(diversity_lambda),
                      torch.from_numpy(score[g].reshape(-1).copy()).to(dev), scores, R, V, bdash if g > 0 else 0, st())
            _lib.call("acvae_topk_flat_batched", scores, V if lt == 0 else bdash * V, bdash * V, bdash, V, vals, idx, prev_d,
                      nxt_d, N, bdash, st())
            top = vals.cpu().numpy().reshape(N, bdash).copy()
            parent_h = prev_d.cpu().numpy().reshape(N, bdash) - base
            nxt_h = nxt_d.cpu().numpy().reshape(N, bdash)
            for i in range(N):
                sq = np.concatenate([seq[i][g][parent_h[i]] if lt > 0 else seq[i][g], nxt_h[i][:, None]], axis=1)
                seq[i][g] = sq
                ended = sq[:, lt] == end_idx
                if lt == T - 1:
                    ended[:] = True
                for b_ in range(bdash):
                    if ended[b_]:
                        done[i][g].append({"seq": sq[b_].copy(), "score": float(top[i, b_]) / (lt + 1)})
                top[i][ended] -= np.float32(1000)
            score[g] = top
            words[g], parents[g] = nxt_d.clone(), prev_d.clone()
    rows = bdash * G if group_nbest else G
    out = np.full((N, rows, T), end_idx, np.int64)
    out_scores = np.zeros((N, rows), np.float64)
    out_lengths = np.zeros((N, rows), np.int32)
    for i in range(N):
        ranked = [sorted(d, key=lambda x: -x["score"])[:bdash] for d in done[i]]
        chosen = sum(ranked, []) if group_nbest else [d[0] for d in ranked]
        for r, beam in enumerate(chosen):
            out[i, r, :len(beam["seq"])] = beam["seq"]
            out_scores[i, r], out_lengths[i, r] = beam["score"], len(beam["seq"])
    return out, out_scores, out_lengths
