"""The doc tower above 128 tokens (csrc/attention_long.hip: key-block walk with an online softmax, fp32 and bf16; the generic kernel for
other head widths) against the reference's own DPRContextEncoder at 512 tokens (g16) and against the CPU oracle.  Every test here needs
L > 128 and fails with GdrError ("L must be <= ...") on a build whose tower stops at 128 tokens."""
import types

import numpy as np
import pytest
import torch

from conftest import golden
from gdr_amd import _ffi, ops, synth
from gdr_amd.config import GDRConfig

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

QB, KB = ops.ATTN_LONG_QUERY_BLOCK, ops.ATTN_LONG_KEY_BLOCK


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _tiny512(**kw):
    return dict(synth.bert_config(True), max_pos=512, **kw)


def _tower(bc, sd, dev, **kw):
    from gdr_amd.modeling import EncoderModel
    return EncoderModel.from_state_dict(bc, sd, dev, **kw)


def _oracle(sd, bc, ids_n, mask_n, **kw):
    from oracle import bert_ref
    hid, pooled = bert_ref.bert_forward(sd, bc, torch.from_numpy(ids_n), torch.from_numpy(mask_n), **kw)
    return hid.numpy(), pooled.numpy()


def _tokens_with_lengths(lens, L, vocab, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    lens = np.asarray(lens)
    ids = g.integers(2, vocab, size=(len(lens), L)).astype(np.int64)
    mask = (np.arange(L)[None, :] < lens[:, None]).astype(np.int64)
    ids[np.arange(len(lens)), lens - 1] = 1
    return ids * mask, mask


# ------------------------------------------------------------------------------------------------------------ 1. reference golden
@pytest.mark.parametrize("name,tol", [("tiny", 1e-4), ("base", 2e-4)])
def test_long_doc_tower_vs_reference_golden(dev, name, tol):
    """g16: the reference's DPRContextEncoder at L = 512 (tiny: 6 passages of 174..512 tokens; bert-base: 512 and 506), padded and ragged
    entry, at the doc tower's own tolerances (test_doc_tower_vs_reference_golden: 1e-4 tiny, 2e-4 base)."""
    g = golden("g16_doc_tower_long")
    bc = _tiny512() if name == "tiny" else synth.bert_config(False)
    enc = _tower(bc, synth.make_bert_state_dict(bc, seed=int(g["seed"])), dev)
    ids_n, mask_n, rows = g[name + "_ids"].astype(np.int64), g[name + "_mask"].astype(np.int64), g[name + "_rows"]
    ids, mask = torch.from_numpy(ids_n).to(dev), torch.from_numpy(mask_n).to(dev)
    live = mask_n[:, rows] != 0
    for ragged in (False, True):
        hid, pooled = enc.bert.forward(ids, mask, ragged=ragged)
        _, pooled_only = enc.bert.forward(ids, mask, ragged=ragged, want_hidden=False)
        got = hid[:, torch.from_numpy(rows).to(dev)].cpu().numpy()
        dp, dh = np.abs(pooled.cpu().numpy() - g[name + "_pooled"]).max(), np.abs(got - g[name + "_hidden"])[live].max()
        print(f"g16 {name} ragged={ragged}: max |pooled - reference| {dp:.2e}, |hidden - reference| (live rows) {dh:.2e}")
        np.testing.assert_allclose(pooled.cpu().numpy(), g[name + "_pooled"], rtol=tol, atol=tol)
        np.testing.assert_allclose(pooled_only.cpu().numpy(), g[name + "_pooled"], rtol=tol, atol=tol)
        np.testing.assert_allclose(got[live], g[name + "_hidden"][live], rtol=tol, atol=tol)
        if ragged:
            assert int((hid[torch.from_numpy(mask_n == 0).to(dev)] != 0).sum()) == 0, "PAD rows of the ragged form must be zero"


# ------------------------------------------------------------------------------------------------------------ 2. edges
def _edge_lengths(L):
    lens = {1, 16, 17, L // 2, L - 1, L}
    for blk in (KB, QB):
        for m in range(blk, L + 2, blk):
            lens |= {x for x in (m - 1, m, m + 1) if 1 <= x < L}
    return sorted(lens)


@pytest.mark.parametrize("L", [129, 130, 144, 145, 160, 192, 193, 255, 256, 257, 320, 384, 511, 512])
def test_long_doc_tower_block_edges_vs_oracle(dev, L):
    """Tiny config (2 heads of 64) with max_pos = 512 against the CPU oracle at 1e-4: sequence lengths 1, 16, 17, L/2, L-1, L and one
    before / on / after every multiple of the kernel's key block and query block.  The padded entry takes the batch as it is; the
    packed kernels only run from 192 GEMM tiles on (bert.hip), so the ragged entry gets the same lengths repeated up to that size."""
    bc = _tiny512()
    sd = synth.make_bert_state_dict(bc, seed=77)
    enc = _tower(bc, sd, dev)
    lens = _edge_lengths(L)
    reps = -(-(192 * 128 + 128) // (len(lens) * L))                  # rows >= 192 tiles of 128: the packed form
    for ragged, ln in ((False, lens), (True, lens * reps)):
        ids_n, mask_n = _tokens_with_lengths(ln, L, bc["vocab_size"], seed=1000 + L)
        ids, mask = torch.from_numpy(ids_n).to(dev), torch.from_numpy(mask_n).to(dev)
        hid, pooled = enc.bert.forward(ids, mask, ragged=ragged, live_rows_hint=int(mask_n.sum()) if ragged else -1)
        rh, rp = _oracle(sd, bc, ids_n, mask_n)
        keep = mask_n != 0
        got = hid.cpu().numpy()
        print(f"L={L} ragged={ragged} B={len(ln)}: max |pooled - oracle| {np.abs(pooled.cpu().numpy() - rp).max():.2e}, "
              f"|hidden - oracle| (live) {np.abs(got - rh)[keep].max():.2e}")
        np.testing.assert_allclose(pooled.cpu().numpy(), rp, rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(got[keep], rh[keep], rtol=1e-4, atol=1e-4)
        if ragged:
            assert not got[~keep].any()


# ------------------------------------------------------------------------------------------------------------ 3. ragged == padded
@pytest.mark.parametrize("B,L", [(24, 384), (8, 512)])
def test_long_ragged_form_is_bit_identical_to_the_padded_form(dev, B, L):
    """test_doc_tower_ragged_form_is_bit_identical_to_the_padded_form above 128 tokens: bert-base, lengths uniform 16..L, one mask that is
    not a prefix of ones (keeps every position and its mask), one full-length passage."""
    bc = synth.bert_config(False)
    enc = _tower(bc, synth.make_bert_state_dict(bc, seed=77), dev)
    ids_n, mask_n = synth.make_tokens(B, L=L, vocab_hi=bc["vocab_size"], seed=9, min_len=16)
    mask_n[5, 10] = 0
    mask_n[7, :] = 1
    ids, mask = torch.from_numpy(ids_n).to(dev), torch.from_numpy(mask_n).to(dev)
    hp, pp = enc.bert.forward(ids, mask, ragged=False)
    hr, pr = enc.bert.forward(ids, mask, ragged=True, live_rows_hint=int(mask_n.sum()))
    _, po = enc.bert.forward(ids, mask, ragged=True, want_hidden=False)
    assert torch.equal(pr, pp) and torch.equal(po, pp), "pooled output of the ragged form differs from the padded form"
    keep = torch.from_numpy(mask_n != 0).to(dev)
    keep[5, :] = True
    assert torch.equal(hr[keep], hp[keep])
    assert int((hr[~keep] != 0).sum()) == 0
    assert float(hp[~keep].abs().max()) > 0             # the padded form did compute those rows


# ------------------------------------------------------------------------------------------------------------ 4. mask shapes
def test_long_mask_with_a_hole_and_all_zero_mask_vs_oracle(dev):
    """Padded form, tiny, L = 384: a mask whose hole covers keys 128..255 entirely (two whole key blocks of masked keys between live
    ones), a mask whose first 64 keys are masked (a masked block in front of the first live key), and a mask that is all zero — the
    additive -1e9 rule makes that sequence the uniform average over all L keys, as in the reference."""
    bc = _tiny512()
    sd = synth.make_bert_state_dict(bc, seed=77)
    enc = _tower(bc, sd, dev)
    L = 384
    ids_n, mask_n = _tokens_with_lengths([L, L, L, L, 200], L, bc["vocab_size"], seed=3)
    mask_n[1, 128:256] = 0
    mask_n[2, :] = 0
    mask_n[3, :64] = 0
    ids, mask = torch.from_numpy(ids_n).to(dev), torch.from_numpy(mask_n).to(dev)
    rh, rp = _oracle(sd, bc, ids_n, mask_n)
    for ragged in (False, True):                          # sequences 1-3 are not prefixes of ones: the ragged form keeps them whole
        hid, pooled = enc.bert.forward(ids, mask, ragged=ragged)
        got = hid.cpu().numpy()
        for b in range(4):
            print(f"mask case {b} ragged={ragged}: max |hidden - oracle| {np.abs(got[b] - rh[b]).max():.2e}")
            np.testing.assert_allclose(got[b], rh[b], rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(pooled.cpu().numpy(), rp, rtol=1e-4, atol=1e-4)


# ------------------------------------------------------------------------------------------------------------ 5. peaked softmax
def test_long_peaked_softmax_vs_oracle(dev):
    """bert-base on the g16 base inputs with every query weight and bias multiplied by 6 (score std 6, mean top probability 0.58): rows
    whose maximum arrives in a late key block carry real weight, so a rescale applied twice or not at all shows.  2e-4 against the
    oracle; the reference and the oracle, two fp32 CPU implementations, differ by 2.2e-5 (pooled) / 3.0e-5 (hidden) on these inputs.
    Padded on the two passages; ragged on four copies of them (4 096 rows: the packed kernels)."""
    g = golden("g16_doc_tower_long")
    bc = synth.bert_config(False)
    sd = synth.make_bert_state_dict(bc, seed=int(g["seed"]))
    for k in list(sd):
        if "attention.self.query." in k:
            sd[k] = sd[k] * 6.0
    enc = _tower(bc, sd, dev)
    ids_n, mask_n, rows = g["base_ids"].astype(np.int64), g["base_mask"].astype(np.int64), g["base_rows"]
    rh, rp = _oracle(sd, bc, ids_n, mask_n)
    for ragged, reps in ((False, 1), (True, 4)):
        ids = torch.from_numpy(np.tile(ids_n, (reps, 1))).to(dev)
        mask = torch.from_numpy(np.tile(mask_n, (reps, 1))).to(dev)
        hid, pooled = enc.bert.forward(ids, mask, ragged=ragged)
        got = hid[:, torch.from_numpy(rows).to(dev)].cpu().numpy()
        want_h, want_p = np.tile(rh[:, rows], (reps, 1, 1)), np.tile(rp, (reps, 1))
        live = np.tile(mask_n[:, rows] != 0, (reps, 1)) if ragged else np.ones(got.shape[:2], bool)   # ragged: PAD rows are zero
        print(f"peaked softmax ragged={ragged}: max |pooled - oracle| {np.abs(pooled.cpu().numpy() - want_p).max():.2e}, "
              f"|hidden - oracle| {np.abs(got - want_h)[live].max():.2e}")
        np.testing.assert_allclose(pooled.cpu().numpy(), want_p, rtol=2e-4, atol=2e-4)
        np.testing.assert_allclose(got[live], want_h[live], rtol=2e-4, atol=2e-4)
        assert not got[~live].any()


# ------------------------------------------------------------------------------------------------------------ 6. bf16 mode
def test_long_bf16_mode_vs_oracle_emulation(dev):
    """test_doc_tower_bf16_mode_vs_oracle_emulation at L = 512 with that test's caps: against the fp32 oracle max <= 1.5e-1 and
    cosine >= 0.9995 for every passage; against bert_ref.bert_forward(bf16=True) max <= 3e-2, mean <= 4e-3.  The kernel splits its
    probabilities exactly into three bf16 pieces (as the 128-token kernel does), so the running maximum adds no rounding point."""
    bc = synth.bert_config(False)
    sd = synth.make_bert_state_dict(bc, seed=77)
    ids_n, mask_n = synth.make_tokens(8, L=512, vocab_hi=bc["vocab_size"], seed=10, min_len=130)
    ids, mask = torch.from_numpy(ids_n).to(dev), torch.from_numpy(mask_n).to(dev)
    e16 = _tower(bc, sd, dev, dtype=torch.bfloat16)
    p16 = e16(passage={"input_ids": ids, "attention_mask": mask}).cpu()
    h16, p16b = e16.bert.forward(ids, mask)
    assert float((p16b.cpu() - p16).abs().max()) < 1e-5
    assert int((h16[torch.from_numpy(mask_n == 0).to(dev)] != 0).sum()) == 0
    emu = torch.from_numpy(_oracle(sd, bc, ids_n, mask_n, bf16=True)[1])
    ref = torch.from_numpy(_oracle(sd, bc, ids_n, mask_n)[1])
    d_emu, d_ref = (p16 - emu).abs(), (p16 - ref).abs()
    cos = torch.nn.functional.cosine_similarity(p16, ref, dim=1)
    print(f"bf16 doc tower at 512 tokens: max |gpu - emulation| {float(d_emu.max()):.3e} (mean {float(d_emu.mean()):.3e}); "
          f"max |gpu - fp32| {float(d_ref.max()):.3e}; emulation vs fp32 {float((emu - ref).abs().max()):.3e}; min cosine {float(cos.min()):.6f}")
    assert float(d_emu.max()) <= 3e-2 and float(d_emu.mean()) <= 4e-3
    assert float(d_ref.max()) <= 1.5e-1
    assert float(cos.min()) >= 0.9995, cos


@pytest.mark.parametrize("L", [129, 192, 257, 512])
def test_long_bf16_mode_block_edges_vs_emulation(dev, L):
    """The bf16 kernel's block edges on the tiny config against the emulation.  Bound: the bert-base caps of the test above (3e-2 max,
    4e-3 mean) — two blocks accumulate less rounding than twelve, so they hold a fortiori; PAD rows zero."""
    bc = _tiny512()
    sd = synth.make_bert_state_dict(bc, seed=77)
    e16 = _tower(bc, sd, dev, dtype=torch.bfloat16)
    ids_n, mask_n = _tokens_with_lengths(_edge_lengths(L), L, bc["vocab_size"], seed=2000 + L)
    ids, mask = torch.from_numpy(ids_n).to(dev), torch.from_numpy(mask_n).to(dev)
    hid, pooled = e16.bert.forward(ids, mask)
    eh, ep = _oracle(sd, bc, ids_n, mask_n, bf16=True)
    keep = mask_n != 0
    d = np.abs(hid.cpu().numpy() - eh)[keep]
    print(f"bf16 tiny L={L}: max |hidden - emulation| {d.max():.3e} (mean {d.mean():.3e}), pooled {np.abs(pooled.cpu().numpy() - ep).max():.3e}")
    assert d.max() <= 3e-2 and d.mean() <= 4e-3 and np.abs(pooled.cpu().numpy() - ep).max() <= 3e-2
    assert not hid.cpu().numpy()[~keep].any()


# ------------------------------------------------------------------------------------------------------------ 7. split form
def test_long_split_form_keeps_fp32_level_embeddings(dev):
    """bert-base split=True (fp16 x 2 linears, the fp32 attention), 8 passages at L = 512: pooled within 5e-5 of the fp32 ragged form
    (the existing split test's number) and within 2e-4 of the oracle."""
    bc = synth.bert_config(False)
    sd = synth.make_bert_state_dict(bc, seed=77)
    ids_n, mask_n = synth.make_tokens(8, L=512, vocab_hi=bc["vocab_size"], seed=10, min_len=130)
    ids, mask = torch.from_numpy(ids_n).to(dev), torch.from_numpy(mask_n).to(dev)
    p32 = _tower(bc, sd, dev, ragged=True)(passage={"input_ids": ids, "attention_mask": mask})
    esp = _tower(bc, sd, dev, split=True)
    psp = esp(passage={"input_ids": ids, "attention_mask": mask})
    hsp, psp2 = esp.bert.forward(ids, mask)
    diff = float((psp - p32).abs().max())
    print(f"fp16 x 2 doc tower at 512 tokens: max |pooled - fp32 pooled| = {diff:.2e}")
    assert diff <= 5e-5 and float((psp2 - psp).abs().max()) <= 1e-5
    assert int((hsp[torch.from_numpy(mask_n == 0).to(dev)] != 0).sum()) == 0
    np.testing.assert_allclose(psp.cpu().numpy(), _oracle(sd, bc, ids_n, mask_n)[1], rtol=2e-4, atol=2e-4)


# ------------------------------------------------------------------------------------------------------------ 8. other widths, refusals
def test_long_other_head_width_vs_oracle(dev):
    """hidden 128 with 8 heads (d_kv = 16) at L = 300: the generic kernel (K and V of a head fit in LDS at this width), padded and
    through the ragged entry, against the oracle at 1e-4."""
    bc = _tiny512(num_heads=8)
    sd = synth.make_bert_state_dict(bc, seed=77)
    enc = _tower(bc, sd, dev)
    ids_n, mask_n = synth.make_tokens(6, L=300, vocab_hi=bc["vocab_size"], seed=21, min_len=3)
    mask_n[0, :] = 1
    ids, mask = torch.from_numpy(ids_n).to(dev), torch.from_numpy(mask_n).to(dev)
    rh, rp = _oracle(sd, bc, ids_n, mask_n)
    keep = mask_n != 0
    for ragged in (False, True):
        hid, pooled = enc.bert.forward(ids, mask, ragged=ragged)
        np.testing.assert_allclose(pooled.cpu().numpy(), rp, rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(hid.cpu().numpy()[keep], rh[keep], rtol=1e-4, atol=1e-4)


def test_long_refusals_name_the_limit(dev):
    def run(bc, L, **kw):
        enc = _tower(bc, synth.make_bert_state_dict(bc, seed=77), dev, **kw)
        ids_n, mask_n = synth.make_tokens(2, L=L, vocab_hi=bc["vocab_size"], seed=5, min_len=L)
        return enc.bert.forward(torch.from_numpy(ids_n).to(dev), torch.from_numpy(mask_n).to(dev))

    for kw in ({}, {"ragged": True}, {"dtype": torch.bfloat16}, {"split": True}):
        with pytest.raises(_ffi.GdrError, match=r"L=513.*512"):
            run(dict(synth.bert_config(True), max_pos=600), 513, **kw)
        with pytest.raises(_ffi.GdrError, match=r"L=200.*max_pos = 160"):
            run(synth.bert_config(True), 200, **kw)
    # d_kv = 128 at L = 512: K and V of a head need 540 KB of LDS in the generic kernel, and only d_kv = 64 has the key-block form
    with pytest.raises(_ffi.GdrError, match=r"d_kv=128 at L=512"):
        run(dict(synth.bert_config(True), hidden_size=256, num_heads=2, max_pos=512), 512)
    hid, _ = run(_tiny512(), 512)                                   # and the tower is usable after the refusals
    assert bool(torch.isfinite(hid).all())


# ------------------------------------------------------------------------------------------------------------ 9. consumers
def _args(V, R=4, **kw):
    return types.SimpleNamespace(num_return_sequences=R, output_vocab_size=V, max_output_length=kw.pop("max_output_length", 3),
                                 length_penalty=0.8, kary=V, position=1, score_rate=kw.pop("score_rate", [0, 1.0]), loss_func="tanh")


def test_add_documents_from_300_token_passages(dev):
    """GDRRetriever.add_documents(tokens=) with 300-token passages: the rows stored in doc_embed are a direct EncoderModel call's."""
    from gdr_amd import codec
    from gdr_amd.modeling import GDRRetriever
    bc = _tiny512()
    tower = _tower(bc, synth.make_bert_state_dict(bc, seed=77), dev)
    d = bc["hidden_size"]
    rng = np.random.default_rng(2)
    N0, C_ = 600, 50
    idx = codec.ClusterIndex(["%d-%d" % (c // 30, c % 30) for c in range(C_)], (np.arange(C_ + 1) * 12).astype(np.int32),
                             rng.permutation(N0).astype(np.int32))
    D0 = torch.from_numpy(rng.standard_normal((N0, d)).astype(np.float32)).to(dev)
    tok0, msk0 = (torch.from_numpy(a).to(dev) for a in synth.make_tokens(N0, L=24, vocab_hi=bc["vocab_size"], seed=4))
    tok, msk = (torch.from_numpy(a).to(dev) for a in synth.make_tokens(40, L=300, vocab_hi=bc["vocab_size"], seed=6, min_len=100))
    direct = tower(passage={"input_ids": tok, "attention_mask": msk})
    r = GDRRetriever(None, D0.clone(), idx, _args(30), doc_tower=tower, doc_tokens=(tok0, msk0))
    r.add_documents(tokens=(tok, msk))
    assert torch.equal(r.doc_embed[N0:], direct) and torch.equal(r.doc_embed[:N0], D0)
    assert r.doc_tokens[0].shape == (N0 + 40, 300) and torch.equal(r.doc_tokens[0][N0:], tok) and torch.equal(r.doc_tokens[1][N0:], msk)
    assert torch.equal(r._reencode(torch.arange(N0, N0 + 40, dtype=torch.int32, device=dev)), direct)


def test_two_stage_with_reencode_of_300_token_passages_vs_oracle(dev):
    """test_two_stage_with_reencode_vs_oracle (tests/test_gpu_decode.py) with 300-token passages: validation_step_i(reencode=True)
    embeds the candidates with the doc tower and ranks them as the oracle composition bert_ref + rerank does."""
    from gdr_amd import codec
    from gdr_amd.modeling import GDRModel, GDRRetriever
    from oracle import beam_ref, codec_ref, retrieval_ref
    bc = _tiny512()
    cfg = GDRConfig.tiny(d_model=128, d_kv=32, num_heads=4, d_ff=256)
    sd, bsd = synth.make_state_dict(cfg, seed=6), synth.make_bert_state_dict(bc, seed=7)
    last = f"{synth.BERT_PREFIX}encoder.layer.{bc['num_layers'] - 1}.output.LayerNorm."
    bsd[last + "weight"], bsd[last + "bias"] = bsd[last + "weight"] * 0.008, bsd[last + "bias"] * 0.008   # keep q.d of order 1 (tanh)
    V = cfg.output_vocab_size
    B, R, csize, Lp = 2, 4, 3, 300
    ids, mask = synth.make_tokens(B, L=10, vocab_hi=cfg.vocab_size, seed=13, min_len=2)
    (rd, rs), enc_x = beam_ref.generate(sd, cfg, torch.from_numpy(ids), torch.from_numpy(mask), R, restricted_head=True)
    dec = codec_ref.dec_2d(codec_ref.decode_token(rd.numpy(), output_vocab_size=V, kary=V), R)
    names = sorted({s for row in dec for s in row}) + ["filler-a", "filler-b"]
    N = len(names) * csize
    offsets = (np.arange(len(names) + 1) * csize).astype(np.int32)
    members = np.random.Generator(np.random.PCG64(4)).permutation(N).astype(np.int32)
    ptok, pmask = synth.make_tokens(N, L=Lp, vocab_hi=bc["vocab_size"], seed=19, min_len=100)
    args = _args(V, R, max_output_length=cfg.max_output_length, score_rate=[0, 1, 3])
    tower = _tower(bc, bsd, dev)
    retr = GDRRetriever(GDRModel(cfg, sd, dev), None, codec.ClusterIndex(names, offsets, members), args, doc_tower=tower,
                        doc_tokens=(torch.from_numpy(ptok).to(dev), torch.from_numpy(pmask).to(dev)))
    out = retr.validation_step_i({"source_ids": torch.from_numpy(ids).to(dev), "source_mask": torch.from_numpy(mask).to(dev)},
                                 reencode=True)
    assert out["clusters"] == dec
    Dref = torch.from_numpy(_oracle(bsd, bc, ptok, pmask)[1])
    direct = tower(passage={"input_ids": torch.from_numpy(ptok).to(dev), "attention_mask": torch.from_numpy(pmask).to(dev)})
    np.testing.assert_allclose(direct.cpu().numpy(), Dref.numpy(), rtol=1e-4, atol=1e-4)
    look = {n: i for i, n in enumerate(names)}
    mem_q = [[m for s in row for m in members[offsets[look[s]]:offsets[look[s] + 1]].tolist()] for row in dec]
    ref = retrieval_ref.rerank(enc_x[::R][:, 0], Dref, mem_q, [[csize] * R] * B, np.array(rs, np.float32).reshape(B, R).tolist(),
                               args.score_rate, R)
    for b in range(B):
        for a in range(len(args.score_rate)):
            assert out["doc_ids"][b][a] == [str(x) for x in ref[b][a][1].tolist()]
