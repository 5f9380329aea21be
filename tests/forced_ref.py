"""Shared by tests/test_forced_host.py and tests/test_gpu_forced.py: the restatement of what the score mode of gdr_t5_generate
(out_len = NULL, include/gdr_hip.h) and the row-query rerank (GDR_RERANK_ROW_QUERIES) compute, from pieces of the CPU oracle that are only
imported.  The reference runs the full model over the decoded rows with decoder_input_ids = outs (main_models.py:1467-1571); a row's
positions up to its first EOS see no PAD key, so the oracle's causal decoder equals that masked forward there, and nothing behind the
first EOS is reported.  No test lives here."""
import numpy as np
import torch

from oracle import t5_ref

torch.set_grad_enabled(False)

PAD, EOS = 0, 1


def first_eos(ids):
    """Per row of ids [rows, ml]: the position of the first EOS at t >= 1, ml for a row without one."""
    ids = np.asarray(ids)
    ml = ids.shape[1]
    hit = ids[:, 1:] == EOS
    return np.where(hit.any(axis=1), hit.argmax(axis=1) + 1, ml)


def counted(ids):
    """The positions the masked mean runs over (main_models.py:1469-1476): t = 0 and every t >= 1 with ids[t] != PAD.  bool[rows, ml]"""
    m = np.asarray(ids) != PAD
    m[:, 0] = True
    return m


def scores_from_logits(logits, ids, length_penalty):
    """logits [rows, ml - 1, Vd] (masked columns -1e9) of positions 0 .. ml-2 -> float64[rows]: the sum over the positions before the
    row's first EOS of log_softmax(logits_t)[ids[t + 1]] — the EOS' own included — over len ** length_penalty, len = the EOS position
    or ml (BeamHypotheses.add, generation_utils.py:1070-1084; the open beams at max_length, :862-883)."""
    ids = np.asarray(ids)
    rows, ml = ids.shape
    logp = torch.log_softmax(torch.as_tensor(logits).double(), dim=-1).numpy()
    eos = first_eos(ids)
    out = np.zeros(rows, np.float64)
    for r in range(rows):
        s = 0.0
        for t in range(min(int(eos[r]), ml - 1)):
            s += logp[r, t, ids[r, t + 1]]
        out[r] = s / float(eos[r]) ** length_penalty
    return out


def planes_from_hidden(h, ids):
    """h [rows, ml, d] last hidden states -> (trace [ml, rows, d] with zeros behind the first EOS, the state at the first EOS [rows, d]
    (zero row without one), the masked mean [rows, d]: the sum over the counted positions, ascending, then one division)."""
    h = np.asarray(h)
    ids = np.asarray(ids)
    rows, ml, d = h.shape
    eos = first_eos(ids)
    trace = np.zeros((ml, rows, d), h.dtype)
    at_eos = np.zeros((rows, d), h.dtype)
    mean = np.zeros((rows, d), h.dtype)
    cnt = counted(ids)
    for r in range(rows):
        for t in range(ml):
            if t <= eos[r]:
                trace[t, r] = h[r, t]
            if cnt[r, t]:
                mean[r] = mean[r] + h[r, t]
        if eos[r] < ml:
            at_eos[r] = h[r, eos[r]]
        mean[r] = mean[r] / h.dtype.type(cnt[r].sum())
    return trace, at_eos, mean


def all_logits(sd, cfg, ids, enc_rows, mask_rows):
    """(h [rows, ml, d], logits [rows, ml - 1, Vd]) of the decode branch over given rows (modeling_t5.py:1529-1646): the causal decoder
    at every position, and per position t < ml - 1 the adaptor head restricted to its live columns — the same numbers as head_full,
    and under t5_ref.bf16_linears() the head GEMM rounds like every other linear — or, for an adaptor-free config, lm_head alone
    (fp32 also in the bf16 mode, include/gdr_hip.h)."""
    ids = torch.as_tensor(ids)
    ml = ids.shape[1]
    h = t5_ref.decoder_forward(sd, cfg, ids, enc_rows, mask_rows)
    if cfg.has_adaptor:
        a = t5_ref.adaptor_forward(sd, cfg, ids)
        lg = torch.stack([t5_ref.head_last_restricted(sd, cfg, h[:, t], a[:, t], t) for t in range(ml - 1)], dim=1)
    else:
        lg = (h[:, :ml - 1] * (cfg.d_model ** -0.5)) @ sd["lm_head.weight"].T
        lg = lg + t5_ref.positional_mask(ml - 1, cfg.decode_vocab_size, cfg.output_vocab_size, lg.dtype)[None]
    return h, lg


def score(sd, cfg, enc_hidden, enc_mask, ids, rows_per_query, length_penalty):
    """What ops.T5DecoderHandle.score(..., hidden=True) returns, as numpy: (scores float64[rows], trace, at_eos, mean) in sd's dtype.
    enc_hidden [B, L, d], enc_mask [B, L]; row b * rows_per_query + r of ids belongs to query b."""
    enc_rows = torch.as_tensor(enc_hidden).repeat_interleave(rows_per_query, dim=0)
    mask_rows = torch.as_tensor(enc_mask).repeat_interleave(rows_per_query, dim=0)
    h, lg = all_logits(sd, cfg, ids, enc_rows, mask_rows)
    return (scores_from_logits(lg, ids, length_penalty),) + planes_from_hidden(h.numpy(), ids)


def rerank_row_queries(q_rows, doc_embed, members, seg_lens, beam_scores, alphas, k, func="tanh"):
    """retrieval_ref.rerank with a query vector per (query, segment) — main_models.py:1588-1594: candidate c of segment j of query b is
    scored against q_rows[b * R + j].  members[b]: the query's candidate doc ids (segments concatenated), seg_lens[b]: R lengths,
    beam_scores [B, R].  float64.  Returns (values [B, A, k], ids [B, A, k]); -inf / -1 pad a query with fewer than k candidates."""
    q = np.asarray(q_rows, np.float64)
    D = np.asarray(doc_embed, np.float64)
    bs = np.asarray(beam_scores, np.float32)
    B, R = bs.shape
    f = np.tanh if func == "tanh" else (lambda x: 1.0 / (1.0 + np.exp(-x)))
    prob = torch.softmax(torch.from_numpy(bs), dim=-1).double().numpy()
    vals = np.full((B, len(alphas), k), -np.inf)
    idx = np.full((B, len(alphas), k), -1, np.int64)
    for b in range(B):
        mem = np.asarray(members[b], np.int64)
        seg = np.repeat(np.arange(R), np.asarray(seg_lens[b], np.int64))
        assert seg.size == mem.size
        sim = f((q[b * R + seg] * D[mem]).sum(-1)) if mem.size else np.zeros(0)
        for ai, alpha in enumerate(alphas):
            s = sim + alpha * prob[b][seg]
            order = np.argsort(-s, kind="stable")[:k]
            vals[b, ai, :order.size] = s[order]
            idx[b, ai, :order.size] = mem[order]
    return vals, idx
