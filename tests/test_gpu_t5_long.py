"""The T5 query tower and generate() above 128 input tokens (csrc/attention_long.hip: the key-block self-attention with T5's relative
position bias and the key-block cross-attention of the beam rows; the generic kernel for other head widths) against the reference's
own T5Stack / generate() (g17) and against the CPU oracle.  Every test here calls an entry point with L > 128, which a build whose T5
entry points stop at 128 tokens refuses with GdrError.  Configs, token batches, the generate() cases and their committed seeds live in
tests/t5_long.py; tolerances are the ones the short-L tests use (test_gpu_parity.py TOL = 1e-4, 2e-4 at t5-base widths;
test_generate_tiny_vs_oracle: ids equal, scores 1e-4; the bf16 encoder test's caps; the split test's 1e-4 / 5e-5)."""
import types

import numpy as np
import pytest
import torch

import t5_long
from conftest import golden, hypothesis_lists_match, beam_cut_explains_absence
from gdr_amd import _ffi, ops, synth
from gdr_amd.config import GDRConfig

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL = 1e-4
QB, KB = ops.ATTN_LONG_QUERY_BLOCK, ops.ATTN_LONG_KEY_BLOCK


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def enc64(dev):
    return ops.T5EncoderHandle(t5_long.t64(), t5_long.state_dict("t64"), dev)


@pytest.fixture(scope="module")
def enc_base2(dev):
    return ops.T5EncoderHandle(t5_long.base2(), t5_long.state_dict("base2"), dev)


def _oracle_enc(kind, ids_n, mask_n, sd=None):
    from oracle import t5_ref
    return t5_ref.encoder_forward(sd or t5_long.state_dict(kind), t5_long.CONFIGS[kind](), torch.from_numpy(ids_n),
                                  torch.from_numpy(mask_n)).numpy()


def _both_forms_vs(enc, dev, ids_n, mask_n, ref, tol, what):
    """Padded and ragged entry against `ref` [B, L, d] on the kept rows (every row of a sequence whose mask is no prefix of ones)."""
    ids, mask = torch.from_numpy(ids_n).to(dev), torch.from_numpy(mask_n).to(dev)
    keep = mask_n != 0
    for b in range(len(mask_n)):
        n = int(mask_n[b].sum())
        if n == 0 or not mask_n[b, :n].all():
            keep[b] = True
    for ragged in (False, True):
        hid, pooled = enc.forward(ids, mask, ragged=ragged, live_rows_hint=int(mask_n.sum()) if ragged else -1)
        got = hid.cpu().numpy()
        print(f"{what} ragged={ragged}: max |hidden - ref| over kept rows {np.abs(got - ref)[keep].max():.2e}")
        np.testing.assert_allclose(got[keep], ref[keep], rtol=tol, atol=tol)
        np.testing.assert_allclose(pooled.cpu().numpy(), ref[:, 0], rtol=tol, atol=tol)
        if ragged:
            assert not got[~keep].any(), "PAD rows of the ragged form must be zero"


# ================================================================================================================ encoder
def test_long_encoder_vs_reference_golden(dev, enc64):
    """1. g17: the reference's T5Stack on t64 at B = 3, L = 300 with 300 / 131 / 17 tokens, padded and ragged entry."""
    g = golden("g17_t5_long")
    assert int(g["seed"]) == t5_long.SD_SEED
    ids_n, mask_n = g["enc_ids"].astype(np.int64), g["enc_mask"].astype(np.int64)
    ref = np.zeros(ids_n.shape + (128,), np.float32)
    ref[mask_n != 0] = g["enc_hidden_live"]
    _both_forms_vs(enc64, dev, ids_n, mask_n, ref, TOL, "g17")


@pytest.mark.parametrize("L", [129, 130, 191, 192, 193, 255, 256, 257, 320, 383, 384, 385, 448, 511, 512])
def test_long_encoder_block_edges_vs_oracle(dev, enc64, L):
    """2. One before / on / after the key-block (64) and query-block (128) multiples: B = 2, the second sequence shorter than the first
    by a random amount, both forms (2 L >= 256 rows: the ragged entry runs its packed kernels)."""
    short = L - int(np.random.Generator(np.random.PCG64(L)).integers(1, L - 1))
    ids_n, mask_n = t5_long.tokens_with_lengths((L, short), L, 128, seed=2000 + L)
    _both_forms_vs(enc64, dev, ids_n, mask_n, _oracle_enc("t64", ids_n, mask_n), TOL, f"L={L} lengths {L}/{short}")


def _ragged_eq_batch(vocab, seed):
    """Lengths 512 / 129 / 128 / 64 / 5, a left-padded row, a mask with a hole and an all-zero mask at L = 512 (eight rows: the five
    lengths and the three masks that are no prefix of ones, which keep every position in the packed layout)."""
    L = 512
    ids_n, mask_n = t5_long.tokens_with_lengths((512, 129, 128, 64, 5, 512, 512, 512), L, vocab, seed)
    mask_n[5, :200] = 0                 # left-padded: three whole key blocks of masked keys in front of the first live one
    mask_n[6, 130:390] = 0              # a hole that swallows whole key blocks between live ones
    mask_n[7, :] = 0                    # all zero: softmax over the bias differences that survive next to -1e9
    return ids_n, mask_n


@pytest.mark.parametrize("kind,tol", [("t64", TOL), ("base2", 2e-4)])
def test_long_ragged_form_is_bit_identical_to_the_padded_form(dev, kind, tol, enc64, enc_base2):
    """3. torch.equal on pooled and on every kept row at L = 512; t64 packs through the split-K forms, base2 (192 tiles) through the
    un-split ones with the token table.  The three sequences whose mask is no prefix of ones are also held to the oracle."""
    enc = enc64 if kind == "t64" else enc_base2
    ids_n, mask_n = _ragged_eq_batch(min(enc.cfg.vocab_size, 32100), seed=9)
    ids, mask = torch.from_numpy(ids_n).to(dev), torch.from_numpy(mask_n).to(dev)
    hp, pp = enc.forward(ids, mask, ragged=False)
    hr, pr = enc.forward(ids, mask, ragged=True, live_rows_hint=int(mask_n[:5].sum()) + 3 * 512)
    _, po = enc.forward(ids, mask, ragged=True, want_hidden=False)
    assert torch.equal(pr, pp) and torch.equal(po, pp), "pooled output of the ragged form differs from the padded form"
    keep = torch.from_numpy(mask_n != 0).to(dev)
    keep[5:] = True
    assert torch.equal(hr[keep], hp[keep])
    assert int((hr[~keep] != 0).sum()) == 0 and float(hp[~keep].abs().max()) > 0
    ref = _oracle_enc(kind, ids_n[5:], mask_n[5:])
    got = hp[5:].cpu().numpy()
    print(f"{kind}: left-padded / hole / all-zero masks, max |hidden - oracle| {np.abs(got - ref).max():.2e}")
    np.testing.assert_allclose(got, ref, rtol=tol, atol=tol)


def test_long_encoder_bias_that_matters(dev):
    """4. The saturated buckets decide: head 0's last bucket of the 'key before query' direction (15) and head 1's last bucket of the
    'key after query' direction (31) sit 6 above the rest, so attention moves onto keys >= 128 positions away — on one side only per
    head, which a wrong bucket or a wrong sign of the offset turns around."""
    from oracle import t5_ref
    cfg, sd = t5_long.t64(), dict(t5_long.state_dict("t64"))
    key = "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"
    w = sd[key].clone()
    w[15, 0] = w[:, 0].max() + 6.0
    w[31, 1] = w[:, 1].max() + 6.0
    sd[key] = w
    ids_n, mask_n = t5_long.tokens_with_lengths((400, 333), 400, cfg.vocab_size, seed=4)
    it, mt = torch.from_numpy(ids_n), torch.from_numpy(mask_n)
    ref, bias = t5_ref.encoder_forward(sd, cfg, it, mt, return_bias=True)
    p = torch.softmax(bias[0, 0, 399, :] + 0.0, -1)
    assert float(p[:272].sum()) > 0.8, "the test's premise: the bias alone puts a late query's weight on keys >= 128 positions before it"
    base = t5_ref.encoder_forward(t5_long.state_dict("t64"), cfg, it, mt)
    assert float((ref - base).abs().max()) > 0.05, "the premise: the raised buckets change the hidden states far beyond the tolerance"
    _both_forms_vs(ops.T5EncoderHandle(cfg, sd, dev), dev, ids_n, mask_n, ref.numpy(), TOL, "raised last buckets")


def test_long_encoder_other_head_widths(dev):
    """5. d_kv = 16 (GDRConfig.tiny) at L = 300 takes the generic kernel (eight 64-key score strips per lane, position bias included);
    d_kv = 128 at L = 512 would need 540 KB of LDS there and has no key-block form: refused, naming d_kv and L."""
    cfg, sd = GDRConfig.tiny(), t5_long.state_dict("tiny")
    ids_n, mask_n = t5_long.tokens_with_lengths((300, 131, 17), 300, cfg.vocab_size, seed=5)
    mask_n[2, :] = 0
    _both_forms_vs(ops.T5EncoderHandle(cfg, sd, dev), dev, ids_n, mask_n, _oracle_enc("tiny", ids_n, mask_n), TOL, "tiny L=300")
    wide = GDRConfig.tiny(d_model=128, d_kv=128, num_heads=2, d_ff=256)
    enc = ops.T5EncoderHandle(wide, synth.make_state_dict(wide, seed=3, with_decoder=False), dev)
    ids_n, mask_n = t5_long.tokens_with_lengths((512, 100), 512, wide.vocab_size, seed=6)
    with pytest.raises(_ffi.GdrError) as e:
        enc.forward(torch.from_numpy(ids_n).to(dev), torch.from_numpy(mask_n).to(dev))
    assert "d_kv=128" in str(e.value) and "L=512" in str(e.value)
    h, _ = enc.forward(torch.from_numpy(ids_n[:, :128]).to(dev), torch.from_numpy(mask_n[:, :128]).to(dev))   # still usable
    assert bool(torch.isfinite(h).all())


@pytest.mark.parametrize("B,ragged", [(3, False), (84, True)])
def test_long_encoder_bf16_mode_vs_oracle_emulation(dev, B, ragged):
    """6a. bf16 precision mode at L = 300: above 128 tokens q / k / v stay fp32 (no bf16 key-block form with position bias), which
    t5_ref.bf16_linears() emulates.  Padded entry, and the packed entry at 84 x 300 rows (192 tiles: its packed kernels).  The caps of
    test_encoder_bf16_mode_vs_oracle_emulation."""
    from oracle import t5_ref
    cfg, sd = t5_long.t64(), t5_long.state_dict("t64")
    ids_n, mask_n = synth.make_tokens(B, L=300, vocab_hi=cfg.vocab_size, seed=B, min_len=100)
    ti, tm = torch.from_numpy(ids_n), torch.from_numpy(mask_n)
    ref32 = t5_ref.encoder_forward(sd, cfg, ti, tm)
    with t5_ref.bf16_linears():
        ref16 = t5_ref.encoder_forward(sd, cfg, ti, tm)
    enc = ops.T5EncoderHandle(cfg, sd, dev, dtype=torch.bfloat16)
    h, pooled = enc.forward(ti.to(dev), tm.to(dev), ragged=ragged)
    keep = tm != 0 if ragged else torch.ones_like(tm, dtype=torch.bool)
    hc, r16, r32 = h.cpu()[keep], ref16[keep], ref32[keep]
    rel = lambda a, b: float((a - b).norm() / b.norm())
    e_emul, e_modes = rel(hc, r16), rel(r32, r16)
    print(f"bf16 mode L=300 ragged={ragged}: |gpu-emul|/|emul| = {e_emul:.2e}, |fp32-emul|/|emul| = {e_modes:.2e}, "
          f"max abs gpu-emul {float((hc - r16).abs().max()):.3e}")
    within_cap = bool(((hc - r16).abs() <= 5e-3 + 5e-3 * r16.abs()).all())
    if not ragged:
        assert within_cap, "the padded form is held to the 5e-3 + 5e-3 |x| cap outright"
    elif not within_cap:
        # The packed case only.  Two correct bf16 implementations differ where a rounding flips (the fp32 values feeding it differ in
        # their last bits), and this case holds 2 x 10^6 elements (measured on an MI355X: 5 of them past the cap, the worst at
        # 7.4e-3).  The cap stays as it is; the case is held to the float64 rule instead: the same emulation with every sum in
        # float64, and the GPU no further from it than twice the fp32 emulation is.
        import peaked
        with t5_ref.bf16_linears():
            r64 = t5_ref.encoder_forward(peaked.as_float64(sd), cfg, ti, tm)[keep]
        e_gpu, e_ref = float((hc.double() - r64).abs().max()), float((r16.double() - r64).abs().max())
        print(f"  past the 5e-3 cap: max |gpu - emul64| {e_gpu:.3e}, max |emul32 - emul64| {e_ref:.3e}")
        assert e_gpu <= 2 * e_ref, (e_gpu, e_ref)
    assert e_emul < 0.5 * e_modes, "the GPU bf16 path must sit much closer to the bf16 emulation than fp32 does"
    torch.testing.assert_close(pooled.cpu(), h.cpu()[:, 0], rtol=0, atol=0)
    torch.testing.assert_close(hc, r32, rtol=1e-1, atol=1e-1)


@pytest.mark.parametrize("split,cap", [(True, 1e-4), (2, 5e-5)])
def test_long_encoder_split_forms_vs_fp32_path(dev, enc64, split, cap):
    """6b. The split forms (six bf16-plane terms; fp16 x 2) run the fp32 key-block attention: pooled and kept rows against the fp32
    path at the existing split test's caps."""
    cfg, sd = t5_long.t64(), t5_long.state_dict("t64")
    ids_n, mask_n = t5_long.tokens_with_lengths((300, 131, 17), 300, cfg.vocab_size, seed=7)
    ids, mask = torch.from_numpy(ids_n).to(dev), torch.from_numpy(mask_n).to(dev)
    h32, p32 = enc64.forward(ids, mask, ragged=True)
    esp = ops.T5EncoderHandle(cfg, sd, dev, split=split)
    hs, ps = esp.forward(ids, mask, ragged=True)
    _, po = esp.forward(ids, mask, ragged=True, want_hidden=False)
    dp, dh = float((ps - p32).abs().max()), float((hs - h32).abs().max())
    print(f"split={split} L=300: max |pooled - fp32| {dp:.2e}, |hidden - fp32| {dh:.2e}")
    assert dp <= cap and float((po - p32).abs().max()) <= cap and dh <= 2e-4
    assert int((hs[torch.from_numpy(mask_n == 0).to(dev)] != 0).sum()) == 0


def test_long_pooled_only_packed_form_over_a_nan_workspace(dev, enc_base2):
    """7. base2 at B = 8, L = 512, pooled only: the packed un-split form with the token table and the last block's Q on the CLS rows.
    Pooled is bit-identical to the padded form with every float of the scratch a NaN before the call."""
    enc = enc_base2
    assert enc.token_table is not None
    ids_n, mask_n = synth.make_tokens(8, L=512, seed=21, min_len=129)
    ids, mask = torch.from_numpy(ids_n).to(dev), torch.from_numpy(mask_n).to(dev)
    _, p0 = enc.forward(ids, mask)
    enc.forward(ids, mask, want_hidden=False, ragged=True)                # the workspace exists now
    torch.cuda.synchronize()
    for buf in enc.ws.bufs.values():
        buf.fill_(255)
    _, p = enc.forward(ids, mask, want_hidden=False, ragged=True, live_rows_hint=int(mask_n.sum()))
    assert bool(torch.isfinite(p).all()) and torch.equal(p, p0)


def test_more_than_512_tokens_is_refused_everywhere(dev, enc64):
    """8. L = 513: every encoder form and generate() name the limit; the handles keep working."""
    from gdr_amd.modeling import GDRModel
    cfg, sd = t5_long.t64(), t5_long.state_dict("t64")
    ids_n, mask_n = t5_long.tokens_with_lengths((513, 20), 513, cfg.vocab_size, seed=8)
    ids, mask = torch.from_numpy(ids_n).to(dev), torch.from_numpy(mask_n).to(dev)
    e16 = ops.T5EncoderHandle(cfg, sd, dev, dtype=torch.bfloat16)
    esp = ops.T5EncoderHandle(cfg, sd, dev, split=True)
    calls = [lambda: enc64.forward(ids, mask), lambda: enc64.forward(ids, mask, ragged=True), lambda: e16.forward(ids, mask),
             lambda: e16.forward(ids, mask, ragged=True), lambda: esp.forward(ids, mask, ragged=True)]
    for dtype in (torch.float32, torch.bfloat16):
        dec = ops.T5DecoderHandle(cfg, sd, dev, dtype=dtype)
        fake = torch.zeros((2, 513, cfg.d_model), device=dev)
        calls.append(lambda dec=dec: dec.generate(fake, mask, 4, cfg.max_output_length, 0.8, 4))
    for call in calls:
        with pytest.raises(_ffi.GdrError) as e:
            call()
        assert "512" in str(e.value), str(e.value)
    h, _ = enc64.forward(ids[:, :512], mask[:, :512])
    ref = _oracle_enc("t64", ids_n[:, :512], mask_n[:, :512])
    np.testing.assert_allclose(h.cpu().numpy(), ref, rtol=TOL, atol=TOL)
    model = GDRModel(cfg, sd, dev)
    (dec, sc), _ = model.generate(ids[:, :512], attention_mask=mask[:, :512], max_length=cfg.max_output_length, num_beams=4,
                                  length_penalty=0.8, num_return_sequences=4, output_scores=True)
    assert np.isfinite(np.array(sc)).all()


# ================================================================================================================ generate()
def _gpu_generate(name, dev, table=False, **model_kw):
    from gdr_amd import codec
    from gdr_amd.modeling import GDRModel
    cfg, sd, ids_n, mask_n, R, ml, use_trie = t5_long.case_inputs(name)
    if use_trie:
        V = cfg.output_vocab_size
        model_kw["trie"] = codec.Trie.from_docids(t5_long.trie_docids(V, use_trie), V)
        if table:
            model_kw["prefix_trie"] = model_kw["trie"]
    model = GDRModel(cfg, sd, dev, **model_kw)
    (dec, sc), _ = model.generate(torch.from_numpy(ids_n).to(dev), attention_mask=torch.from_numpy(mask_n).to(dev), max_length=ml,
                                  num_beams=R, length_penalty=0.8, num_return_sequences=R, output_scores=True)
    return dec.cpu().numpy(), np.array(sc)


def _check_case(name, dev, **model_kw):
    """The oracle's margins first (CPU), then the GPU: ids equal and scores to 1e-4 wherever the oracle's score is finite."""
    rd, rs = t5_long.assert_margins(name)
    dec, sc = _gpu_generate(name, dev, **model_kw)
    rs = np.array(rs)
    fin = np.isfinite(rs) & (rs > -1e8)
    print(f"{name}: {int(fin.sum())}/{len(rs)} finite hypotheses, max |score - oracle| {np.abs(sc[fin] - rs[fin]).max():.2e}")
    np.testing.assert_allclose(sc[fin], rs[fin], rtol=1e-4, atol=1e-4)
    assert np.array_equal(dec[fin], rd.numpy()[fin])


@pytest.mark.parametrize("name", ["t64_129", "t64_300", "t64_512", "t64_200_r100"])
def test_long_generate_vs_oracle(dev, name):
    """9. (B, R, L) = (2, 4, 129), (2, 4, 300), (3, 10, 512) with 512 / 140 / 9 tokens, and (1, 100, 200): infer.sh's beams — seven
    16-row tiles of beam rows per (query, head), slab-sourced q rows at the small ones, one row per query at step 0."""
    _check_case(name, dev)


def test_long_generate_100_beams_plain_weights_tie_aware(dev):
    """9b. (1, 100, 200) on the plain t64 weights, whose 100 final scores lie too close for the margin rule (t5_long.HEAD_SHARP), under
    the tie-aware rule: scores of shared hypotheses within the generate tests' 1e-4, and with that 1e-4 as the tie window (oracle scores
    more than 2e-4 apart cannot swap) every moved or foreign hypothesis must be explained by a tie of the oracle's own search."""
    name = "t64_200_r100_plain"
    cfg, _, ids_n, _, R, _, _ = t5_long.case_inputs(name)
    rd, rs, trace, ptrace, _ = t5_long.oracle(name)
    dec, sc = _gpu_generate(name, dev)
    rs, ref = np.array(rs), rd.numpy()
    assert ids_n.shape[0] == 1 and np.isfinite(rs).all() and (rs > -1e8).all()
    W = min(dec.shape[1], ref.shape[1])
    glist, rlist = [tuple(r[:W]) for r in dec.tolist()], [tuple(r[:W]) for r in ref.tolist()]
    where = {x: i for i, x in enumerate(rlist)}
    gap = max(abs(sc[p] - rs[where[x]]) for p, x in enumerate(glist) if x in where)
    tie = 1e-4
    explain = lambda hyp: beam_cut_explains_absence(trace, ptrace, 0, R, cfg.decode_vocab_size, list(hyp), tie, final_cut=rs[-1])
    moved, foreign, sizes = hypothesis_lists_match(rlist, rs, glist, tie, explain_foreign=explain)
    print(f"{name}: score gap on shared hypotheses {gap:.2e}, {moved} moved, {foreign} foreign, {len(sizes)} tie groups (largest "
          f"{max(sizes)}) over {R} hypotheses")
    assert gap <= 1e-4
    assert len(where.keys() & set(glist)) >= R - 5 and len(sizes) > R // 2, "the rule must not be one big tie group"


@pytest.mark.parametrize("table", [False, True])
def test_long_generate_with_trie_and_prefix_table_vs_oracle(dev, table):
    """10. L = 300 under the trie constraint, without and with the prefix table (GdrPrefixTable) over the same trie."""
    _check_case("t64_300_trie", dev, table=table)


def test_long_generate_bf16_mode_vs_oracle_emulation(dev):
    """11. gdr_t5_generate_bf16 at (B, R, L) = (2, 10, 300): attention stays fp32 and takes the same key-block kernel.  The rule of
    test_generate_bf16_mode_vs_oracle_emulation: the emulation runs on the GPU's own encoder states, the tie window is the measured
    score gap (<= 5e-3), and hypothesis_lists_match raises when two hypotheses outside a tie group swap."""
    from oracle import beam_ref, t5_ref
    cfg, sd = t5_long.t64(), t5_long.state_dict("t64")
    B, R, L, ml = 2, 10, 300, cfg.max_output_length
    ids_n, mask_n = t5_long.tokens_with_lengths((300, 140), L, cfg.vocab_size, seed=11)
    idt, mt = torch.from_numpy(ids_n), torch.from_numpy(mask_n)
    enc16 = ops.T5EncoderHandle(cfg, sd, dev, dtype=torch.bfloat16)
    dec16 = ops.T5DecoderHandle(cfg, sd, dev, dtype=torch.bfloat16)
    enc_h, _ = enc16.forward(idt.to(dev), mt.to(dev), want_pooled=False)
    out_ids, lens, scores, ts, tt = dec16.generate(enc_h, mt.to(dev), R, ml, 0.8, R, trace=True)
    dec, sc = ops.finish_generate_output(out_ids, lens, scores, ml)
    idx = torch.arange(B).view(-1, 1).repeat(1, R).view(-1)
    enc_x, mask_x = enc_h.cpu().index_select(0, idx), mt.index_select(0, idx)

    def step(seq):
        with t5_ref.bf16_linears():
            return t5_ref.decode_logits(sd, cfg, seq, enc_x, mask_x, restricted=True)

    trace, ptrace = [], []
    rd, rs = beam_ref.beam_search(step, B, R, cfg.decode_vocab_size, ml, 0.8, R, trace=trace, prefix_trace=ptrace)
    g0, r0 = ts[0].cpu().numpy(), trace[0][0].numpy()
    live = r0 > -1e8
    np.testing.assert_allclose(g0[live], r0[live], rtol=5e-3, atol=5e-3)
    sc, rs = np.array(sc).reshape(B, R), np.array(rs).reshape(B, R)
    np.testing.assert_allclose(sc, rs, rtol=3e-2, atol=3e-2)
    got, ref = dec.cpu().numpy(), rd.numpy()
    W = min(got.shape[1], ref.shape[1])
    glists = [[tuple(r[:W]) for r in got[b * R:(b + 1) * R].tolist()] for b in range(B)]
    rlists = [[tuple(r[:W]) for r in ref[b * R:(b + 1) * R].tolist()] for b in range(B)]
    gap = 0.0
    for b in range(B):
        where = {x: i for i, x in enumerate(rlists[b])}
        gap = max([gap] + [abs(sc[b, p] - rs[b, where[x]]) for p, x in enumerate(glists[b]) if x in where])
    assert gap <= 5e-3, f"hypothesis scores of the GPU and the emulation differ by {gap:.2e} on shared hypotheses"
    tie = max(gap, 2e-4)
    shared = 0
    for b in range(B):
        def explain(hyp, b=b):
            return beam_cut_explains_absence(trace, ptrace, b, R, cfg.decode_vocab_size, list(hyp), tie, final_cut=rs[b, -1])
        hypothesis_lists_match(rlists[b], rs[b], glists[b], tie, explain_foreign=explain)
        shared += len(set(glists[b]) & set(rlists[b]))
    print(f"bf16 generate L=300: score gap {gap:.2e}, {shared}/{B * R} hypotheses shared")
    assert shared >= 0.8 * B * R


@pytest.mark.parametrize("name", ["tiny_300", "base2_512"])
def test_long_generate_other_widths_vs_oracle(dev, name):
    """12. GDRConfig.tiny() at L = 300: d_kv = 16, the generic kernel serves the beam rows and step 0's single row over 300 keys.
    base2 at (2, 4, 512): twelve heads of 64 at t5-base widths."""
    _check_case(name, dev)


def test_long_queries_through_validation_step(dev):
    """13. GDRRetriever.validation_step_i on t64 with 200-token queries (200 / 131 / 17 tokens): decoded clusters equal the oracle's
    constrained search, and the in-cluster rerank equals the oracle rerank of the oracle's CLS rows."""
    from gdr_amd import codec
    from gdr_amd.modeling import GDRModel, GDRRetriever
    from oracle import codec_ref, retrieval_ref
    name = "t64_200_step"
    cfg, sd, ids_n, mask_n, R, ml, _ = t5_long.case_inputs(name)
    rd, rs = t5_long.assert_margins(name)
    V, csz = cfg.output_vocab_size, 3
    names = ["-".join(str(x) for x in synth.cluster_digits(c, 2, V)) for c in range(V * V)]
    N = len(names) * csz
    offs = (np.arange(len(names) + 1) * csz).astype(np.int32)
    Dn = synth.make_corpus(N, cfg.d_model, cluster_size=csz, seed=8)
    a = types.SimpleNamespace(num_return_sequences=R, output_vocab_size=V, max_output_length=ml, length_penalty=0.8, kary=V,
                              position=1, score_rate=[0, 1.0], loss_func="tanh")
    trie = codec.Trie.from_docids(names, V)                              # = t5_long.trie_docids(V, 1), the case's trie
    model = GDRModel(cfg, sd, dev, trie=trie, prefix_trie=trie)
    idx = codec.ClusterIndex(names, offs, np.arange(N, dtype=np.int32))
    it, mt = torch.from_numpy(ids_n).to(dev), torch.from_numpy(mask_n).to(dev)
    out = GDRRetriever(model, torch.from_numpy(Dn).to(dev), idx, a).validation_step_i({"source_ids": it, "source_mask": mt})
    B = ids_n.shape[0]
    ref_clusters = codec_ref.dec_2d(codec_ref.decode_token(rd.numpy(), output_vocab_size=V, kary=V), R)
    rs = np.array(rs).reshape(B, R)
    q = torch.from_numpy(_oracle_enc("t64", ids_n, mask_n)[:, 0])
    for b in range(B):
        fin = np.isfinite(rs[b])
        assert [c for c, f in zip(out["clusters"][b], fin) if f] == [c for c, f in zip(ref_clusters[b], fin) if f]
        bs = np.array(out["inf_result_batch_prob"], np.float32).reshape(-1, R)[b:b + 1]
        np.testing.assert_allclose(bs[0][fin], rs[b][fin], rtol=1e-4, atol=1e-4)
        mem = [m for s_ in out["clusters"][b] for m in idx[s_]]
        num = [len(idx[s_]) for s_ in out["clusters"][b]]
        ref = retrieval_ref.rerank(q[b:b + 1], torch.from_numpy(Dn), [mem], [num], bs.tolist(), a.score_rate, R)[0]
        for ai in range(2):
            np.testing.assert_allclose(out["rerank_values"][b, ai].cpu().numpy(), ref[ai][0].numpy(), rtol=1e-4, atol=1e-4)
