"""GPU tests of the teacher-forced decode — the score mode of gdr_t5_generate / gdr_t5_generate_bf16 (out_len = NULL; csrc/beam.hip
forced_step_kernel) — of the row-query rerank (GDR_RERANK_ROW_QUERIES) and of the decoder-side stage-2 queries built on both
(--use_query_embed_decoder_special / --use_query_embed_decoder_avg; main_models.py:1467-1594), against tests/forced_ref.py.

Tolerances are those the existing decode tests hold the same oracle to (tests/test_gpu_decode.py): 1e-4 for hypothesis scores, 2e-4 for
hidden states, 3e-2 for the bf16 mode against the bf16_linears emulation; 1e-4 and the tie rule of tests/test_gpu_rerank.py for reranked
lists.  Shapes: B = 3 queries x 5 rows (15 rows: no multiple of 4 or 64), L = 9 with ragged masks, max_length = 5."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

import forced_ref
import peaked
from abi_guard import guarded, guarded_input, poisoned_workspace
from conftest import ranked_lists_match
from gdr_amd import synth
from gdr_amd.config import GDRConfig

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL_SCORE, TOL_HIDDEN, TOL_BF16, TOL_RERANK = 1e-4, 2e-4, 3e-2, 1e-4
B, R, L, LP = 3, 5, 9, 0.8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ cases
def _cfg(kind):
    over = dict(adaptor_ff=128)                                                     # every dim a multiple of 8: the bf16 linears take it
    if kind.startswith("kv64"):                                                     # d_kv = 64: the ancestor / MFMA attention forms
        over.update(d_model=128, d_kv=64, num_heads=2, d_ff=256)
    if kind.endswith("plain"):
        over.update(adaptor_decode=0, adaptor_efficient=0)
    return GDRConfig.tiny(**over)


def given_rows(cfg, rows_per_query, seed=11):
    """Hand-built rows [B * rows_per_query, max_length]: START, digits of positions 0, 1, ..., EOS, PAD — EOS at positions 1, 2, ...,
    max_length - 1 and none at all, in turn; row 2 carries at position 0 a token that belongs to position 2 (no live column there) and
    row 1 at position 0 the FIRST digit token of position 1, V + 2: one past position 0's last live digit, where a column index that
    is off by one would meet the EOS column."""
    V, ml = cfg.output_vocab_size, cfg.max_output_length
    g = np.random.Generator(np.random.PCG64(seed))
    rows = np.zeros((B * rows_per_query, ml), np.int64)
    for r in range(rows.shape[0]):
        eos = 1 + r % ml                                                           # ml: no EOS
        for t in range(1, ml):
            rows[r, t] = (t - 1) * V + 2 + int(g.integers(0, V)) if t < eos else (1 if t == eos else 0)
    if rows.shape[0] > 2:
        rows[2, 1] = 2 * V + 2 + 1
    rows[1, 1] = V + 2
    return rows


@functools.lru_cache(maxsize=None)
def _case(kind, rows_per_query, bf16):
    """(cfg, sd, query tokens, mask, given rows): everything of a case that lives on the host."""
    cfg = _cfg(kind)
    sd = synth.make_state_dict(cfg, seed=1234)
    ids, mask = synth.make_tokens(B, L=L, vocab_hi=cfg.vocab_size, seed=5, min_len=3)
    return cfg, sd, ids, mask, given_rows(cfg, rows_per_query)


_REF = {}


def _run(dev, kind, rows_per_query=R, bf16=False):
    """The handle's answer and the oracle's for one case; the oracle's is computed once per case and shared."""
    from gdr_amd import ops
    cfg, sd, ids, mask, rows = _case(kind, rows_per_query, bf16)
    dt = torch.bfloat16 if bf16 else torch.float32
    enc = ops.T5EncoderHandle(cfg, sd, dev)
    dec = ops.T5DecoderHandle(cfg, sd, dev, dtype=dt)
    mt = torch.from_numpy(mask).to(dev)
    enc_h, _ = enc.forward(torch.from_numpy(ids).to(dev), mt, want_pooled=False)
    key = (kind, rows_per_query, bf16)
    if key not in _REF:
        if bf16:
            with forced_ref.t5_ref.bf16_linears():
                _REF[key] = forced_ref.score(sd, cfg, enc_h.cpu(), torch.from_numpy(mask), rows, rows_per_query, LP)
        else:
            _REF[key] = forced_ref.score(sd, cfg, enc_h.cpu(), torch.from_numpy(mask), rows, rows_per_query, LP)
    return cfg, dec, enc_h, mt, rows, _REF[key]


CASES = [("tiny", R, False), ("tiny_plain", R, False), ("kv64", R, False), ("kv64_plain", R, False), ("tiny", 1, False),
         ("tiny", R, True), ("tiny_plain", R, True), ("kv64", R, True)]


@pytest.mark.parametrize("kind,rows_per_query,bf16", CASES, ids=[f"{k}-{n}rows-{'bf16' if b else 'f32'}" for k, n, b in CASES])
def test_scores_and_hidden_states_of_given_rows_match_the_oracle(dev, kind, rows_per_query, bf16):
    cfg, dec, enc_h, mt, rows, (rs, rtrace, reos, rmean) = _run(dev, kind, rows_per_query, bf16)
    ml, n = cfg.max_output_length, rows.shape[0]
    rows_d = torch.from_numpy(rows).to(dev)
    keep = rows_d.clone()
    scores, trace, at_eos, mean = dec.score(enc_h, mt, rows_d, rows_per_query, LP, hidden=True)
    alone = dec.score(enc_h, mt, rows_d, rows_per_query, LP)
    assert torch.equal(rows_d, keep), "the given rows are an input"
    assert scores.dtype == torch.float64 and tuple(scores.shape) == (n,) and tuple(trace.shape) == (ml, n, cfg.d_model)
    assert torch.equal(alone, scores), "the scores do not depend on whether the hidden states are wanted"
    got_s, got_t, got_e, got_m = (x.cpu().numpy() for x in (scores, trace, at_eos, mean))
    ts, th = (TOL_BF16, TOL_BF16) if bf16 else (TOL_SCORE, TOL_HIDDEN)
    print(f"{kind} {rows_per_query} bf16={bf16}: max |score - ref| {np.abs(got_s - rs)[np.abs(rs) < 1e8].max():.3g}, "
          f"max |hidden - ref| {np.abs(got_t - rtrace).max():.3g}, eos plane {np.abs(got_e - reos).max():.3g}, "
          f"mean plane {np.abs(got_m - rmean).max():.3g}")
    np.testing.assert_allclose(got_s, rs, rtol=ts, atol=ts)
    np.testing.assert_allclose(got_t, rtrace, rtol=th, atol=th)
    np.testing.assert_allclose(got_e, reos, rtol=th, atol=th)
    np.testing.assert_allclose(got_m, rmean, rtol=th, atol=th)
    eos = forced_ref.first_eos(rows)
    assert (eos == ml).any() and all((eos == p).any() for p in range(1, ml)) or rows_per_query == 1
    for r in range(n):
        assert not got_t[eos[r] + 1:, r].any(), f"row {r}: positions behind the first EOS are zero"
        if eos[r] == ml:
            assert not got_e[r].any(), f"row {r}: no EOS, the EOS plane is a zero row"
        else:
            assert np.array_equal(got_e[r], got_t[eos[r], r])
    # the rows with a token outside its position's live columns, the boundary token (t + 1) * V + 2 among them: the masked logit, -1e9
    for r in (1, 2):
        assert rs[r] < -1e8 and got_s[r] < -1e8, r
    assert np.isfinite(got_s).all() and (got_s[3:] > -1e8).all()


@pytest.mark.parametrize("kind", ["tiny", "kv64_plain"])
@pytest.mark.parametrize("constrained", [True, False], ids=["trie", "free"])
def test_scoring_what_generate_returned_reproduces_its_scores(dev, kind, constrained):
    """No oracle: generate()'s hypotheses (with the trie every one ends in EOS, at depth 1, 2 or 3; without it random weights mostly
    never emit EOS) scored as given rows give generate()'s out_scores.  The weights are peaked (tests/peaked.py): the head discriminates,
    the hypotheses' scores are far apart.  Step 0 of a search computes one row per query, the score mode one per hypothesis, and the
    fp32 linears choose their split by the row count: the sums need not be bit-identical.  Held to 1e-4; DESIGN §16 records the
    observed maximum."""
    from gdr_amd import codec
    from gdr_amd.modeling import GDRModel
    cfg = _cfg(kind)
    sd = peaked.peaked_t5(synth.make_state_dict(cfg, seed=1234), cfg, peaked.MODERATE.s, peaked.MODERATE.rb, peaked.MODERATE.hs)
    V = cfg.output_vocab_size
    g = np.random.Generator(np.random.PCG64(9))
    docids = sorted({"-".join(str(int(x)) for x in g.integers(0, V, size=int(g.integers(1, 4)))) for _ in range(80)})
    trie = codec.Trie.from_docids(docids, V) if constrained else None
    model = GDRModel(cfg, sd, dev, trie=trie)
    ids, mask = synth.make_tokens(B, L=L, vocab_hi=cfg.vocab_size, seed=7, min_len=3)
    it, mt = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)
    enc_h, rows, lens, scores = model._generate_launch(it, mt, R, cfg.max_output_length, LP, R)
    again = model.dec.score(enc_h, mt, rows, R, LP)
    via_model = model.score_docids(it, rows, attention_mask=mt, length_penalty=LP)
    assert torch.equal(again, via_model)
    s0, s1 = scores.cpu().numpy(), again.cpu().numpy()
    assert np.isfinite(s0).all(), "every query returned num_beams hypotheses"
    eos = forced_ref.first_eos(rows.cpu().numpy())
    if constrained:
        assert (eos < cfg.max_output_length).all() and len(set(eos.tolist())) > 1, "hypotheses that end at varying depth"
    else:
        assert (eos == cfg.max_output_length).any(), "hypotheses that never end"
    print(f"{kind} {'trie' if constrained else 'free'}: max |score(generate's rows) - generate's score| = {np.abs(s0 - s1).max():.3g}")
    np.testing.assert_allclose(s1, s0, rtol=TOL_SCORE, atol=TOL_SCORE)


# ------------------------------------------------------------------------------------------------ rerank with a query row per segment
SEGS = (1, 3, 0, 5, 18)     # segments straddle the wave's 4 candidates and the workgroup's 16; one is empty


def _lists(seg_lens, n_docs, seed):
    """Per query: candidate doc ids (distinct) and the R segment lengths; then both layouts."""
    g = np.random.Generator(np.random.PCG64(seed))
    members = [g.permutation(n_docs)[:sum(s)].astype(np.int32) for s in seg_lens]
    csr_off = np.concatenate([[0], np.cumsum([n for s in seg_lens for n in s])]).astype(np.int32)
    csr_ids = np.concatenate(members).astype(np.int32)
    stride = 32
    blk_off = np.stack([np.concatenate([[0], np.cumsum(s)]) for s in seg_lens]).astype(np.int32)
    blk_ids = np.full((len(seg_lens), stride), -1, np.int32)
    for b, m in enumerate(members):
        blk_ids[b, :m.size] = m
    return members, {"csr": (csr_off, csr_ids, 0), "blocks": (blk_off, blk_ids, stride)}


@functools.lru_cache(maxsize=None)
def _rerank_inputs(Rr):
    n_docs, d = 300, 64
    seg_lens = [list(np.roll(SEGS, b)) for b in range(B)] if Rr == len(SEGS) else [[7], [1], [20]]
    members, layouts = _lists(seg_lens, n_docs, seed=21)
    D = synth.make_corpus(n_docs, d, cluster_size=3, seed=8)
    g = np.random.Generator(np.random.PCG64(4))
    q = (g.standard_normal((B, d)) * 1.5).astype(np.float32)
    q_rows = (g.standard_normal((B * Rr, d)) * 1.5).astype(np.float32)
    beam = -np.sort(g.random((B, Rr)).astype(np.float32) * 2.0, axis=1)
    return seg_lens, members, layouts, D, q, q_rows, beam


@pytest.mark.parametrize("Rr", [len(SEGS), 1], ids=["R5", "R1"])
@pytest.mark.parametrize("layout", ["csr", "blocks"])
def test_row_queries_with_equal_rows_are_the_one_query_rerank_bit_for_bit(dev, layout, Rr):
    from gdr_amd import ops
    seg_lens, members, layouts, D, q, q_rows, beam = _rerank_inputs(Rr)
    off, ids, stride = layouts[layout]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)                 # noqa: E731
    Dd, qd, rep = t(D), t(q), t(np.repeat(q, Rr, axis=0))
    alphas, k = [0.0, 0.5, 1.0], 6
    forms = {"plain": dict(), "chunked": dict(chunked=True), "positions": dict(positions=True), "sigmoid": dict(func="sigmoid"),
             "doc_range": dict(doc_range=(40, 260)), "bf16": dict()}
    for name, kw in forms.items():
        corpus = Dd.to(torch.bfloat16) if name == "bf16" else (Dd[40:260].contiguous() if name == "doc_range" else Dd)
        args = (corpus, t(off), t(ids), t(beam), alphas, k)
        v0, i0 = ops.rerank_topk(qd, *args, cand_stride=stride, max_cand=27, **kw)
        v1, i1 = ops.rerank_topk(rep, *args, cand_stride=stride, max_cand=27, row_queries=True, **kw)
        assert torch.equal(v0, v1) and torch.equal(i0, i1), (name, layout)
        assert bool((i0 >= 0).any())
    with pytest.raises(ops._ffi.GdrError):                                             # q must hold B * R rows
        ops.rerank_topk(qd if Rr > 1 else rep[:2], Dd, t(off), t(ids), t(beam), alphas, k, cand_stride=stride, max_cand=27, row_queries=True)


@pytest.mark.parametrize("Rr", [len(SEGS), 1], ids=["R5", "R1"])
@pytest.mark.parametrize("layout", ["csr", "blocks"])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16corpus"])
def test_row_queries_with_distinct_rows_match_the_restatement(dev, layout, Rr, bf16):
    from gdr_amd import ops
    seg_lens, members, layouts, D, q, q_rows, beam = _rerank_inputs(Rr)
    off, ids, stride = layouts[layout]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)                 # noqa: E731
    Dd = t(D).to(torch.bfloat16) if bf16 else t(D)
    Dref = Dd.to(torch.float32).cpu().numpy()                                       # the bf16 corpus' own values: widening is exact
    alphas, k = [0.0, 1.0], 6
    for func in ("tanh", "sigmoid"):
        v, i = ops.rerank_topk(t(q_rows), Dd, t(off), t(ids), t(beam), alphas, k, func=func, cand_stride=stride, max_cand=27, row_queries=True)
        rv, ri = forced_ref.rerank_row_queries(q_rows, Dref, members, seg_lens, beam, alphas, k, func=func)
        v, i = v.cpu().numpy(), i.cpu().numpy()
        for b in range(B):
            for a in range(len(alphas)):
                kk = min(k, len(members[b]))
                np.testing.assert_allclose(v[b, a, :kk], rv[b, a, :kk], rtol=TOL_RERANK, atol=TOL_RERANK)
                ranked_lists_match(ri[b, a, :kk].tolist(), rv[b, a, :kk], i[b, a, :kk].tolist(), TOL_RERANK)
                assert (i[b, a, kk:] == -1).all()
    # the rows matter: the one-query call over the same lists ranks differently
    v1, _ = ops.rerank_topk(t(q), Dd, t(off), t(ids), t(beam), alphas, k, cand_stride=stride, max_cand=27)
    assert not np.allclose(v1.cpu().numpy(), v, atol=1e-3)


# ------------------------------------------------------------------------------------------------ end to end: the decoder-side stage 2
def _retriever(dev, cfg, sd, constrained=True, **flags):
    from gdr_amd import codec
    from gdr_amd.modeling import GDRModel, GDRRetriever
    V, csz = cfg.output_vocab_size, 3
    names = ["-".join(str(x) for x in synth.cluster_digits(c, 2, V)) for c in range(V * V)]
    N = len(names) * csz
    offs = (np.arange(len(names) + 1) * csz).astype(np.int32)
    Dn = synth.make_corpus(N, cfg.d_model, cluster_size=csz, seed=8)
    a = types.SimpleNamespace(num_return_sequences=4, output_vocab_size=V, max_output_length=cfg.max_output_length, length_penalty=LP,
                              kary=V, position=1, score_rate=[0, 1.0], loss_func="tanh", **flags)
    full = codec.Trie.from_docids(names, V)
    model = GDRModel(cfg, sd, dev, trie=full, prefix_trie=full) if constrained else GDRModel(cfg, sd, dev)
    idx = codec.ClusterIndex(names, offs, np.arange(N, dtype=np.int32))
    return GDRRetriever(model, torch.from_numpy(Dn).to(dev), idx, a), model, idx, Dn, a


@pytest.mark.parametrize("form", ["special", "avg"])
def test_validation_step_with_decoder_side_queries_matches_the_restatement(dev, form):
    """Stage 2 scored against each hypothesis' own decoder vector: the step's lists against forced_ref.rerank_row_queries fed with the
    planes forced_ref.score computes for the step's hypotheses — nothing of the restatement comes from the score mode."""
    cfg = GDRConfig.tiny()
    sd = synth.make_state_dict(cfg, seed=1234)
    flags = {"use_query_embed_encoder": 0, "use_query_embed_decoder_" + form: 1}
    if form == "special":
        flags["use_query_embed_decoder_avg"] = 1                                    # both set: `special` wins
    retr, model, idx, Dn, a = _retriever(dev, cfg, sd, **flags)
    assert retr.query_form == form
    ids, mask = synth.make_tokens(4, L=12, vocab_hi=cfg.vocab_size, seed=5, min_len=3)
    it, mt = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)
    out = retr.validation_step_i({"source_ids": it, "source_mask": mt})
    Rn = a.num_return_sequences
    enc_h, rows, lens, scores = model._generate_launch(it, mt, Rn, a.max_output_length, LP, Rn)
    _s, _t, at_eos, mean = forced_ref.score(sd, cfg, enc_h.cpu(), torch.from_numpy(mask), rows.cpu().numpy(), Rn, LP)
    q_rows = at_eos if form == "special" else mean
    assert (forced_ref.first_eos(rows.cpu().numpy()) < a.max_output_length).all()
    mem = [[m for s_ in out["clusters"][b] for m in idx[s_]] for b in range(4)]
    num = [[len(idx[s_]) for s_ in out["clusters"][b]] for b in range(4)]
    bs = np.array(out["inf_result_batch_prob"], np.float32).reshape(-1, Rn)
    rv, ri = forced_ref.rerank_row_queries(q_rows, Dn, mem, num, bs, a.score_rate, Rn)
    v, i = out["rerank_values"].cpu().numpy(), out["doc_id_tensor"].cpu().numpy()
    for b in range(4):
        for ai in range(2):
            np.testing.assert_allclose(v[b, ai], rv[b, ai], rtol=TOL_RERANK, atol=TOL_RERANK)
            ranked_lists_match(ri[b, ai].tolist(), rv[b, ai], i[b, ai].tolist(), TOL_RERANK)
    # and it is another ranking than the encoder-CLS one
    base = _retriever(dev, cfg, sd)[0].validation_step_i({"source_ids": it, "source_mask": mt})
    assert out["clusters"] == base["clusters"] and not torch.equal(base["rerank_values"], out["rerank_values"])


def test_validation_step_without_the_flags_is_what_it_was(dev):
    cfg = GDRConfig.tiny()
    sd = synth.make_state_dict(cfg, seed=1234)
    ids, mask = synth.make_tokens(4, L=12, vocab_hi=cfg.vocab_size, seed=5, min_len=3)
    batch = {"source_ids": torch.from_numpy(ids).to(dev), "source_mask": torch.from_numpy(mask).to(dev)}
    plain = _retriever(dev, cfg, sd)[0].validation_step_i(batch)
    stated = _retriever(dev, cfg, sd, use_query_embed_encoder=1, use_query_embed_decoder_special=0,
                        use_query_embed_decoder_avg=0)[0].validation_step_i(batch)
    for k_ in ("rerank_values", "doc_id_tensor"):
        assert torch.equal(plain[k_], stated[k_])
    assert plain["clusters"] == stated["clusters"] and plain["inf_result_batch_prob"] == stated["inf_result_batch_prob"]
    # the same lists from the one-query rerank called directly over the step's candidates: nothing but the encoder-CLS path ran
    from gdr_amd import ops
    retr, model, idx, Dn, a = _retriever(dev, cfg, sd)
    enc_h, rows, lens, scores = model._generate_launch(batch["source_ids"], batch["source_mask"], 4, a.max_output_length, LP, 4)
    _cl, offs, dev_ids, stride = retr._device_index().candidates(rows, 4, 4)
    v, i = ops.rerank_topk(enc_h[:, 0].contiguous(), retr.doc_embed, offs, dev_ids, scores.to(torch.float32).view(4, 4), a.score_rate, 4,
                           max_cand=ops.block_max_cand(offs, 4, stride, cap=ops.RERANK_LONG_MAX_CAND), cand_stride=stride)
    assert torch.equal(v, plain["rerank_values"]) and torch.equal(i, plain["doc_id_tensor"])


def test_special_refuses_hypotheses_without_eos(dev):
    from gdr_amd import _ffi
    cfg = GDRConfig.tiny()
    sd = synth.make_state_dict(cfg, seed=1234)
    retr, model, idx, Dn, a = _retriever(dev, cfg, sd, constrained=False, use_query_embed_encoder=0, use_query_embed_decoder_special=1)
    ids, mask = synth.make_tokens(4, L=12, vocab_hi=cfg.vocab_size, seed=5, min_len=3)
    it, mt = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)
    rows = model._generate_launch(it, mt, 4, a.max_output_length, LP, 4)[1]
    n_open = int((forced_ref.first_eos(rows.cpu().numpy()) == a.max_output_length).sum())
    assert n_open > 0, "the unconstrained random model leaves hypotheses without EOS"
    with pytest.raises(_ffi.GdrError) as e:
        retr.validation_step_i({"source_ids": it, "source_mask": mt})
    assert f"{n_open} of {rows.shape[0]}" in str(e.value) and "EOS" in str(e.value)
    # the mean needs no EOS
    avg = _retriever(dev, cfg, sd, constrained=False, use_query_embed_encoder=0, use_query_embed_decoder_avg=1)[0]
    out = avg.validation_step_i({"source_ids": it, "source_mask": mt})            # (few of these rows name a cluster of the index)
    assert tuple(out["rerank_values"].shape) == (4, 2, 4) and not bool(torch.isnan(out["rerank_values"]).any())


# ------------------------------------------------------------------------------------------------ the mode's memory contract
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["tiny", "tiny_plain"])
def test_score_mode_memory_contract(dev, kind, bf16):
    """A workspace of exactly gdr_t5_generate_workspace_bytes and step_scores of exactly (max_length + 2) * rows * d floats between guard
    bands, the scratch poisoned with two fills, on a non-default stream: nothing outside is written, the inputs (out_ids among them) are
    unchanged, and the results do not depend on what the scratch held."""
    from gdr_amd import ops
    from gdr_amd.ops import lib, ptr
    cfg, dec, enc_h, mt, rows, _ref = _run(dev, kind, R, bf16)
    ml, d, n = cfg.max_output_length, cfg.d_model, rows.shape[0]
    NAN = float("nan")
    Ed, eh = guarded_input(enc_h.cpu(), tail=torch.full((8 * L, d), NAN))
    Md, mh = guarded_input(mt.cpu().to(torch.int64), tail=torch.ones(8 * L, dtype=torch.int64))
    Id, ih = guarded_input(torch.from_numpy(rows), tail=torch.ones(8 * ml, dtype=torch.int64))
    need = lib().gdr_t5_generate_workspace_bytes(C.byref(dec.struct), B, L, R, ml)
    fn = lib().gdr_t5_generate_bf16 if bf16 else lib().gdr_t5_generate
    stream = torch.cuda.Stream(device=dev)
    results = []
    for fill in (0x00, 0xFF, 0x5A):
        ws, wh = poisoned_workspace(need, fill, dev)
        sc, sh = guarded((n,), torch.float64, dev)
        pl, ph = guarded((ml + 2, n, d), torch.float32, dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            rc = fn(C.byref(dec.struct), ptr(Ed), ptr(Md), B, L, R, ml, LP, R, None, None, ptr(Id), None, ptr(sc), ptr(pl), None,
                    ptr(ws), need, ops.stream_ptr())
        assert rc == 0, lib().gdr_last_error()
        stream.synchronize()
        for h_, what in ((wh, "workspace"), (sh, "out_scores"), (ph, "step_scores")):
            h_.check(what)
        for h_, what in ((eh, "enc_hidden"), (mh, "enc_mask"), (ih, "out_ids")):
            h_.unchanged(what)
        results.append((sc.clone(), pl.clone()))
    for s_, p_ in results[1:]:
        assert torch.equal(s_, results[0][0]) and torch.equal(p_, results[0][1]), "the result depends on what the scratch held"
    assert not bool(torch.isnan(results[0][1]).any())
    s_ops, tr, e_, m_ = dec.score(enc_h, mt, torch.from_numpy(rows).to(dev), R, LP, hidden=True)
    assert torch.equal(s_ops, results[0][0]) and torch.equal(torch.cat([tr, e_[None], m_[None]]), results[0][1]), "differs from the ops path"
    # one byte short
    ws, wh = poisoned_workspace(need, 0, dev)
    assert fn(C.byref(dec.struct), ptr(Ed), ptr(Md), B, L, R, ml, LP, R, None, None, ptr(Id), None, ptr(results[0][0]), None, None,
              ptr(ws), need - 1, ops.stream_ptr()) == ops._ffi.GDR_ENOSPC


@pytest.mark.parametrize("kind", ["tiny", "kv64_plain"])
def test_score_mode_in_a_captured_graph_replayed_with_other_rows(dev, kind):
    """The call holds no host synchronisation and joins its side stream: captured once, replayed after out_ids changed, it gives what an
    eager call gives for the new rows."""
    from gdr_amd import ops
    from gdr_amd.ops import lib, ptr
    cfg, dec, enc_h, mt, rows, _ref = _run(dev, kind, R, False)
    ml, d, n = cfg.max_output_length, cfg.d_model, rows.shape[0]
    other = np.ascontiguousarray(rows[::-1])
    mask64 = mt.to(torch.int64).contiguous()
    need = lib().gdr_t5_generate_workspace_bytes(C.byref(dec.struct), B, L, R, ml)
    s_ids = torch.from_numpy(rows).to(dev)
    s_ws = torch.empty(need, dtype=torch.uint8, device=dev)
    s_sc = torch.empty(n, dtype=torch.float64, device=dev)
    s_pl = torch.empty((ml + 2, n, d), dtype=torch.float32, device=dev)

    def call():
        ops.check(lib().gdr_t5_generate(C.byref(dec.struct), ptr(enc_h), ptr(mask64), B, L, R, ml, LP, R, None, None, ptr(s_ids), None,
                                        ptr(s_sc), ptr(s_pl), None, ptr(s_ws), need, ops.stream_ptr()), "gdr_t5_generate")
    warm = torch.cuda.Stream(device=dev)                     # capture needs one eager run first (the side-stream lease, lazy loads)
    warm.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(warm):
        call()
    torch.cuda.current_stream().wait_stream(warm)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for given in (rows, other, rows):
        s_ids.copy_(torch.from_numpy(given).to(dev))
        s_sc.fill_(7.0)
        s_pl.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        es, et, ee, em = dec.score(enc_h, mt, torch.from_numpy(given).to(dev), R, LP, hidden=True)
        assert torch.equal(s_sc, es) and torch.equal(s_pl, torch.cat([et, ee[None], em[None]]))
