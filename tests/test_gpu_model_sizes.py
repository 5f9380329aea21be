"""The kernels at the widths the CLI offers beyond t5-base: `--model_info small` (d 512, 8 heads, d_ff 2048, 6 / 3 layers) and
`--model_info large` (d 1024, 16 heads, d_ff 4096, 24 / 12 layers), built exactly as main.py builds them
(GDRConfig.from_args(parsers_parser([...]))), and the doc tower at bert-large widths (hidden 1024, 16 heads, d_ff 4096).  The
launchers pick their forms by shape, so these widths run code the base-size tests never reach: the split linears' virtual
contraction length below 2 048 (d 512 with 3 terms or fp16 x 2: no plane epilogue), the adaptor at head width 64 / 128, the
similarity kernels at their d <= 1024 limits.  Linears and similarity scores are held against float64, end-to-end paths against the
fp32 oracle at the tolerance the base-size test of the same path uses.  Depth is cut only where the CPU oracle would dominate (the
decode tests); widths, head counts and d_ff are the CLI's."""
import numpy as np
import pytest
import torch

from conftest import beam_cut_explains_absence, hypothesis_lists_match, order_insensitive_topk_match, ranked_lists_match
from gdr_amd.config import GDRConfig
from gdr_amd import synth

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
TOL = 1e-4
TOL32 = 2e-6          # the pre-filter's exactness rule (test_gpu_prefilter.py): two fp32 summation orders of the same products
SIZES = ("small", "large")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _cfg(size, **depth):
    from gdr_amd.main import parsers_parser
    cfg = GDRConfig.from_args(parsers_parser(["--model_info", size]))
    for k, v in depth.items():
        setattr(cfg, k, v)
    return cfg


@pytest.fixture(scope="module")
def models():
    """Per-module cache of the state dicts, handles and bench-batch results (the full-depth t5-large encoder alone is ~1.3 GB on the
    host): built on first use, released when the module's tests are done."""
    cache = {}
    yield cache
    cache.clear()
    torch.cuda.empty_cache()


def _enc(models, size, dev):
    """(cfg, encoder-only state dict, fp32 handle) at the CLI's full depth, built once per module."""
    key = ("enc", size)
    if key not in models:
        from gdr_amd import ops
        cfg = _cfg(size)
        sd = synth.make_state_dict(cfg, seed=1234, with_decoder=False)
        models[key] = (cfg, sd, ops.T5EncoderHandle(cfg, sd, dev))
    return models[key]


def _bench_batch(models, size, dev):
    """The bench batch (512 queries x L 40 = 20 480 token rows), its fp32 pooled output (ragged form) and the oracle's pooled
    vectors on a seeded sample of 16 of the queries (encoder rows do not depend on the other rows of the batch)."""
    key = ("batch", size)
    if key not in models:
        from oracle import t5_ref
        cfg, sd, enc = _enc(models, size, dev)
        ids_n, mask_n = synth.make_tokens(512, L=40, seed=11)
        ids, mask = torch.from_numpy(ids_n).to(dev), torch.from_numpy(mask_n).to(dev)
        _, p32 = enc.forward(ids, mask, want_hidden=False, ragged=True)
        sample = np.sort(np.random.default_rng(17).choice(512, 16, replace=False))
        ref = t5_ref.encoder_forward(sd, cfg, torch.from_numpy(ids_n[sample]), torch.from_numpy(mask_n[sample]))
        models[key] = (ids_n, mask_n, ids, mask, p32, sample, ref)
    return models[key]


# ------------------------------------------------------------------------------------------- a. fp32 encoder
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("B,L", [(2, 1), (3, 33), (2, 128)])
def test_encoder_padded_vs_oracle(dev, models, size, B, L):
    """The padded fp32 encoder at the CLI's widths and depth (6 / 24 layers) against the fp32 oracle at the base-size encoder's
    hidden-state tolerance (2e-4)."""
    from oracle import t5_ref
    cfg, sd, enc = _enc(models, size, dev)
    ids, mask = synth.make_tokens(B, L=L, seed=B * 100 + L, min_len=1)
    ref = t5_ref.encoder_forward(sd, cfg, torch.from_numpy(ids), torch.from_numpy(mask))
    h, pooled = enc.forward(torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev))
    err = float((h.cpu() - ref).abs().max())
    print(f"{size} encoder B={B} L={L}: max |gpu - oracle| = {err:.2e}")
    torch.testing.assert_close(h.cpu(), ref, rtol=2e-4, atol=2e-4)
    assert torch.equal(pooled, h[:, 0])


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("B", [512, 8])
def test_encoder_ragged_bit_identical_to_padded_and_the_oracle_sample(dev, models, size, B):
    """The ragged form at the bench batch (512 x 40 = 20 480 token rows) and at a small batch: pooled and every kept hidden row equal
    the padded form bit for bit (as tests/test_gpu_ragged.py states for base); at 512 the oracle on a seeded sample of 16 queries."""
    cfg, sd, enc = _enc(models, size, dev)
    if B == 512:
        ids_n, mask_n, ids, mask, p32, sample, ref = _bench_batch(models, size, dev)
    else:
        ids_n, mask_n = synth.make_tokens(B, L=40, seed=19, min_len=8)
        ids, mask = torch.from_numpy(ids_n).to(dev), torch.from_numpy(mask_n).to(dev)
    h0, p0 = enc.forward(ids, mask)
    h1, p1 = enc.forward(ids, mask, ragged=True, live_rows_hint=int(mask_n.sum()))
    _, p2 = enc.forward(ids, mask, ragged=True, want_hidden=False)
    assert torch.equal(p1, p0) and torch.equal(p2, p0)
    keep = torch.from_numpy(mask_n != 0).to(dev)
    assert torch.equal(h1[keep], h0[keep])
    assert int((h1[~keep] != 0).sum()) == 0
    if B == 512:
        assert torch.equal(p32, p0)
        got = h0[torch.from_numpy(sample).to(dev)].cpu()
        torch.testing.assert_close(got, ref, rtol=2e-4, atol=2e-4)


# ------------------------------------------------------------------------------------------- b. bf16 precision mode
@pytest.mark.parametrize("size", SIZES)
def test_encoder_bf16_mode_vs_oracle_emulation(dev, models, size):
    """C5 precision mode at the CLI's widths against the oracle's bf16 emulation, under the rule test_gpu_parity's
    test_encoder_bf16_mode_vs_oracle_emulation applies at base (deep stacks: flipped roundings, so norm and worst-element bounds)."""
    from gdr_amd import ops
    from oracle import t5_ref
    cfg, sd, _ = _enc(models, size, dev)
    ids, mask = synth.make_tokens(4, L=40, vocab_hi=cfg.vocab_size, seed=44, min_len=13)
    ti, tm = torch.from_numpy(ids), torch.from_numpy(mask)
    ref32 = t5_ref.encoder_forward(sd, cfg, ti, tm)
    with t5_ref.bf16_linears():
        ref16 = t5_ref.encoder_forward(sd, cfg, ti, tm)
    h, pooled = ops.T5EncoderHandle(cfg, sd, dev, dtype=torch.bfloat16).forward(ti.to(dev), tm.to(dev))
    hc = h.cpu()
    rel = lambda a, b: float((a - b).norm() / b.norm())
    print(f"bf16 mode {size}: |gpu-emul|/|emul| = {rel(hc, ref16):.2e}, |fp32-emul|/|emul| = {rel(ref32, ref16):.2e}, "
          f"max abs gpu-emul {float((hc - ref16).abs().max()):.3e}")
    assert rel(hc, ref16) < 8e-3 and rel(hc, ref32) < 8e-3 and float((hc - ref16).abs().max()) < 6e-2
    torch.testing.assert_close(pooled.cpu(), hc[:, 0], rtol=0, atol=0)


# ------------------------------------------------------------------------------------------- c. split encoder forms
_SPLIT_BOUND = {6: 1e-4, 3: 2e-4, 2: 5e-5}    # pooled vs the fp32 form at the bench batch: test_gpu_parity's bounds for base


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("split", [6, 3, 2])
def test_encoder_split_forms_at_the_bench_batch(dev, models, size, split):
    """gdr_t5_encoder_forward_ragged_split at 512 x 40 (the norms' plane outputs; the wi plane epilogue where the 256-row tile serves
    the virtual contraction length: 6 K0 / 3 K0 >= 2 048 — at d 512 only 6 terms, the 3-term and fp16 x 2 forms store fp32 and split
    in a launch of their own).  Pooled vs the fp32 form within the base-size bounds (6 terms 1e-4, 3 terms 2e-4, fp16 x 2 5e-5);
    the oracle's 16-query sample at 2e-4 (measured: small 8.1e-6 / 4.1e-5 / 4.3e-6, large 1.4e-5 / 5.3e-5 / 7.0e-6 for 6 / 3 / 2
    terms).  Before the routing fix, d 512 with 3 terms / fp16 x 2 fed wo_ff one plain bf16 image read as planes: 7.3e-3 / 3.05."""
    from gdr_amd import ops
    cfg, sd, _ = _enc(models, size, dev)
    ids_n, mask_n, ids, mask, p32, sample, ref = _bench_batch(models, size, dev)
    esp = ops.T5EncoderHandle(cfg, sd, dev, split=split)
    _, psp = esp.forward(ids, mask, want_hidden=False, ragged=True, live_rows_hint=int(mask_n.sum()))
    diff = float((psp - p32).abs().max())
    print(f"{size} split={split}, 512 queries: max |pooled - fp32 pooled| = {diff:.2e}")
    assert diff <= _SPLIT_BOUND[split]
    torch.testing.assert_close(psp[torch.from_numpy(sample).to(dev)].cpu(), ref[:, 0], rtol=2e-4, atol=2e-4)


# ------------------------------------------------------------------------------------------- d. split linear
_PAIRS = {"small": [(1536, 512), (512, 512), (2048, 512), (512, 2048)],
          "large": [(3072, 1024), (1024, 1024), (4096, 1024), (1024, 4096)]}


def _split_linear_check(dev, M, N, K, seed, forms=(6, 3, 2), grow=1.0):
    """Returns the measured errors; asserts the bounds of test_linear_split_bf16_carries_fp32_operands against float64 (the absolute
    ones times `grow`) and that a 130-row launch gives the first 130 rows of the big launch bit for bit, for every form in `forms`."""
    from gdr_amd import ops
    g = torch.Generator().manual_seed(seed)
    a, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5
    A, W = a.to(dev), w.to(dev)
    rows = torch.arange(0, M, max(1, M // 48))[:48]
    ref = a[rows].double() @ w.double().T
    scale = float(ref.abs().mean())
    err = lambda c: float((c[rows.to(dev)].cpu().double() - ref).abs().max()) / scale
    e_f32 = err(ops.linear(A, W))
    out = {"f32": e_f32}
    small = min(M, 130)
    if 6 in forms or 3 in forms:
        Ap, Wp = ops.split_bf16x3(A), ops.split_bf16x3(W)
        for t in (6, 3):
            if t in forms:
                c = ops.linear_split_bf16(Ap, Wp, K, terms=t)
                out[t] = err(c)
                assert torch.equal(c[:small], ops.linear_split_bf16(Ap[:small].contiguous(), Wp, K, terms=t)), t
    if 2 in forms:
        Ah, Wh = ops.split_f16x2(A), ops.split_f16x2(W)
        c = ops.linear_split_bf16(Ah, Wh, K, terms=2)
        out[2] = err(c)
        assert torch.equal(c[:small], ops.linear_split_bf16(Ah[:small].contiguous(), Wh, K, terms=2))
    # the binding bound of each form: absolute (x grow), and for 6 terms / fp16 x 2 relative to the fp32 linear's own error
    bound = {"f32": 3e-5 * grow, 6: min(3e-5 * grow, 3.0 * e_f32 + 1e-6), 3: 1e-4 * grow, 2: min(1.5e-5 * grow, 1.5 * e_f32 + 1e-6)}
    print(f"split linear M={M} N={N} K0={K}: " + ", ".join(f"{k}: {v:.2e} ({v / bound[k]:.0%} of its bound {bound[k]:.2e})"
                                                            for k, v in out.items()))
    for k, v in out.items():
        assert v <= bound[k], (k, out, bound)
    if 6 in out and 3 in out:
        assert out[6] < out[3], out
    return out


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("pair", range(4))
@pytest.mark.parametrize("M", [300, 4100, 12308])
def test_linear_split_at_the_encoder_shapes(dev, size, pair, M):
    """gdr_linear_split_bf16 at every encoder (N, K0) of the size — qkv, o, wi, wo_ff — on 64-row (300), 128-row (4 100) and 256-row
    (12 308, where the virtual K reaches 2 048) tiles, terms 6 / 3 / 2, against float64."""
    N, K = _PAIRS[size][pair]
    _split_linear_check(dev, M, N, K, seed=M + N + K)


@pytest.mark.parametrize("K", [7488, 12800])
@pytest.mark.parametrize("M", [300, 4100])
def test_linear_split_long_contractions_index_the_planes_exactly(dev, K, M):
    """K0 the entry point accepts beyond the model shapes: 7 488 (nk0 = 117 K-tiles per plane block) and 12 800 (nk0 = 200), on the
    64-row and 128-row tiles (one kernel template), against float64.  The block / tile split of a virtual K-tile used to be a reciprocal
    multiply, wrong for 841 of the nk0 in 1 .. 1 024 (the first is 117); it only ever missed the 6-term form's last K-tile (kt 701 at
    nk0 117, kt 1 199 at nk0 200: block 6, tile -1, a read before the operand row) — the 3-term and fp16 x 2 forms stay below it.  fp16 x 2 needs K0 % 128 == 0: 7 488 must be refused, not run.
    The bounds relative to the fp32 MFMA linear's own error are the encoder shapes' (6 terms <= 3x, fp16 x 2 <= 1.5x); the absolute
    ones (fixed at K0 <= 3 072) grow with the fp32 accumulation error, as sqrt(K0 / 3 072): against float64 the fp32 linear itself
    measured 2.1e-5 .. 2.4e-5 of mean |c| at these K0, 6 terms 2.1e-5 .. 3.5e-5 (K0 12 800, 300 rows), fp16 x 2 8.4e-6 .. 9.2e-6 —
    a wrong plane or tile offset gives errors of order 1."""
    from gdr_amd import ops, _ffi
    grow = (K / 3072) ** 0.5
    if K % 128:
        _split_linear_check(dev, M, 2048, K, seed=K + M, forms=(6,), grow=grow)
        A = torch.randn(4, K, device=dev)
        with pytest.raises(_ffi.GdrError):
            ops.linear_split_bf16(ops.split_f16x2(A), ops.split_f16x2(A), K, terms=2)
    else:
        _split_linear_check(dev, M, 2048, K, seed=K + M, forms=(6, 2), grow=grow)


def test_f16x2_operand_range(dev):
    """What the fp16 x 2 form carries (x = hi + lo' 2^-11, hi = fp16(x)) over magnitudes 2^-30 .. 2^17: in [2^-14, 65 520) the planes
    reconstruct x to 2^-21 relative; below fp16's normal range the bound is absolute (3e-11); from 65 520 on hi is infinite and a
    linear over such a row gives a non-finite output row — never a finite wrong value.  Rows of the linear whose operands sit in fp16's
    normal range are held against float64 at |c - ref| <= 2e-5 |a|.|w| per output (22 bits per operand, K = 256 fp32 accumulate);
    rows below it stay finite (their error is printed, not bounded: it depends on fp16 subnormals inside the MFMA)."""
    from gdr_amd import ops
    K, N = 256, 64
    g = torch.Generator().manual_seed(5)
    exps = torch.arange(-30, 18)
    u = (1.0 + 0.99 * torch.rand(len(exps), K, generator=g)) * torch.where(torch.rand(len(exps), K, generator=g) < 0.5, -1.0, 1.0)
    a = (u * torch.pow(2.0, exps.double()).view(-1, 1)).float()
    edge = torch.tensor([65504.0, 65510.0, 65519.0, 65520.0, 65536.0, 2.0 ** -14, 2.0 ** -24, 3e-9])
    x = torch.cat([a.flatten(), edge])
    X = x.to(dev).view(1, -1)
    P = ops.split_f16x2(X)
    n = x.numel()
    hi, lo = P[0, :n].float().cpu(), P[0, n:2 * n].float().cpu()
    rec = hi.double() + lo.double() / 2048.0
    xd, ax = x.double(), x.double().abs()
    normal = (ax >= 2.0 ** -14) & (ax < 65520)
    assert bool(((rec - xd).abs()[normal] <= 2.0 ** -21 * ax[normal]).all())
    assert bool(((rec - xd).abs()[ax < 2.0 ** -14] <= 3e-11).all())
    assert bool((~torch.isfinite(hi[ax >= 65520])).all()) and bool(torch.isfinite(hi[ax < 65520]).all())
    w = torch.randn(N, K, generator=g) * K ** -0.5
    c = ops.linear_split_bf16(ops.split_f16x2(a.to(dev)), ops.split_f16x2(w.to(dev)), K, terms=2).cpu().double()
    ref = a.double() @ w.double().T
    big = (a.abs() >= 65520).any(dim=1)
    assert int(big.sum()) == 2                                           # 2^16 and 2^17
    assert bool((~torch.isfinite(c[big])).all()), "a row with an operand >= 65 520 must not come out finite"
    assert bool(torch.isfinite(c[~big]).all())
    fin = (exps >= -14) & ~big                                           # every operand of the row in fp16's normal range
    bound = 2e-5 * (a.double().abs() @ w.double().abs().T)
    worst = ((c - ref).abs() / bound)
    print("fp16 x 2 linear, |c - ref| / (2e-5 |a|.|w|) per row exponent: " +
          ", ".join(f"2^{int(e)}: {float(worst[j].max()):.2g}" for j, e in enumerate(exps) if not big[j]))
    assert bool((worst[fin] <= 1.0).all()), float(worst[fin].max())


# ------------------------------------------------------------------------------------------- e. generate()
def _gen_model(models, size):
    """Reduced depth (2 encoder, 2 decoder blocks; the CLI's 4 adaptor layers) so that the CPU oracle stays cheap; widths exact."""
    key = ("gen", size)
    if key not in models:
        cfg = _cfg(size, num_layers=2, num_decoder_layers=2)
        models[key] = (cfg, synth.make_state_dict(cfg, seed=31))
    return models[key]


@pytest.mark.parametrize("size,B,R", [("small", 64, 32), ("small", 3, 6), ("large", 2, 10), ("large", 1, 100)])
def test_generate_vs_oracle(dev, models, size, B, R):
    """generate() fp32 against beam_ref.generate, with and without the prefix table: scores at 1e-4, ids by the ranked-list rule.
    small at 64 x 32 = 2 048 beam rows (rows x 8 heads >= 16 384: the four-heads-per-wave attention serves the adaptor, head width
    64); large at head width 128 (the row-group form's upper limit) with infer.sh's beam width 100."""
    from gdr_amd import codec
    from gdr_amd.modeling import GDRModel
    from oracle import beam_ref
    cfg, sd = _gen_model(models, size)
    V = cfg.output_vocab_size
    ids, mask = synth.make_tokens(B, L=16, seed=B + R, min_len=3)
    (rd, rs), _ = beam_ref.generate(sd, cfg, torch.from_numpy(ids), torch.from_numpy(mask), R, restricted_head=True)
    rs = np.array(rs).reshape(B, R)
    names = synth.make_cluster_ids(3000, cluster_size=6, V=V)[0]
    for model in (GDRModel(cfg, sd, dev), GDRModel(cfg, sd, dev, prefix_trie=codec.Trie.from_docids(names, V))):
        (dec, sc), _ = model.generate(torch.from_numpy(ids).to(dev), attention_mask=torch.from_numpy(mask).to(dev),
                                      max_length=cfg.max_output_length, num_beams=R, length_penalty=0.8, num_return_sequences=R,
                                      output_scores=True)
        sc = np.array(sc).reshape(B, R)
        np.testing.assert_allclose(sc, rs, rtol=1e-4, atol=1e-4)
        got, ref = dec.cpu().numpy(), rd.numpy()
        W = min(got.shape[1], ref.shape[1])
        for b in range(B):
            ranked_lists_match([tuple(r[:W]) for r in ref[b * R:(b + 1) * R].tolist()], rs[b],
                               [tuple(r[:W]) for r in got[b * R:(b + 1) * R].tolist()], 1e-4)


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("use_table", [False, True])
def test_generate_bf16_mode_vs_oracle_emulation(dev, models, size, use_table):
    """generate() in the bf16 precision mode (config C5's beam 30: bf16 decoder / adaptor / head linears, the head-dot epilogue with
    dot_d = d_model, the bf16 prefix-table build) at the small / large widths, reduced depth as above, with and without the prefix table.
    The rule of test_gpu_decode.py::test_generate_bf16_mode_vs_oracle_emulation at base: the oracle's bf16 emulation fed the GPU's own
    encoder states; first-step scores to 5e-3; final scores to 3e-2 against the emulation and the fp32 oracle; ids by the tie rule with
    the measured score gap (<= 5e-3) as tie window; >= 95 % of the hypotheses shared; the best one exact when its margin exceeds the tie."""
    from gdr_amd import codec, ops
    from oracle import beam_ref, t5_ref
    cfg, sd = _gen_model(models, size)
    B, R = 2, 30
    V, ml = cfg.output_vocab_size, cfg.max_output_length
    ids, mask = synth.make_tokens(B, L=40, vocab_hi=min(cfg.vocab_size, 32100), seed=6, min_len=3)
    idt, mt = torch.from_numpy(ids), torch.from_numpy(mask)
    enc16 = ops.T5EncoderHandle(cfg, sd, dev, dtype=torch.bfloat16)
    dec16 = ops.T5DecoderHandle(cfg, sd, dev, dtype=torch.bfloat16)
    tab = None
    if use_table:
        names = synth.make_cluster_ids(30000, cluster_size=12, V=V)[0]
        tab = ops.PrefixTable(dec16, codec.Trie.from_docids(names, V), dev)
    enc_h, _ = enc16.forward(idt.to(dev), mt.to(dev), want_pooled=False)
    out_ids, lens, scores, ts, tt = dec16.generate(enc_h, mt.to(dev), R, ml, 0.8, R, trace=True, prefix_table=tab)
    dec, sc = ops.finish_generate_output(out_ids, lens, scores, ml)
    enc_cpu = enc_h.cpu()
    idx = torch.arange(B).view(-1, 1).repeat(1, R).view(-1)
    enc_x, mask_x = enc_cpu.index_select(0, idx), mt.index_select(0, idx)

    def step16(seq):
        with t5_ref.bf16_linears():
            return t5_ref.decode_logits(sd, cfg, seq, enc_x, mask_x, restricted=True)

    trace, ptrace = [], []
    rd, rs = beam_ref.beam_search(step16, B, R, cfg.decode_vocab_size, ml, 0.8, R, trace=trace, prefix_trace=ptrace)
    fd, fs = beam_ref.beam_search(lambda seq: t5_ref.decode_logits(sd, cfg, seq, enc_x, mask_x, restricted=True), B, R,
                                  cfg.decode_vocab_size, ml, 0.8, R)
    g0, r0 = ts[0].cpu().numpy(), trace[0][0].numpy()
    live = r0 > -1e8
    np.testing.assert_allclose(g0[live], r0[live], rtol=5e-3, atol=5e-3)
    sc, rs, fs = np.array(sc).reshape(B, R), np.array(rs).reshape(B, R), np.array(fs).reshape(B, R)
    np.testing.assert_allclose(sc, rs, rtol=3e-2, atol=3e-2)
    np.testing.assert_allclose(sc, fs, rtol=3e-2, atol=3e-2)
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
        if rs[b, 0] - rs[b, 1] > 2 * tie:
            assert glists[b][0] == rlists[b][0]
    print(f"bf16 generate {size} R={R} table={use_table}: score gap {gap:.2e}, {shared}/{B * R} hypotheses shared")
    assert shared >= 0.95 * B * R, (shared, B * R)


# ------------------------------------------------------------------------------------------- f. similarity at d 512 / 1024
def _topk64(Q, D, k):
    s = Q.astype(np.float64) @ D.astype(np.float64).T
    i = np.argsort(-s, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(s, i, 1), i


@pytest.mark.parametrize("d", [512, 1024])
@pytest.mark.parametrize("B", [96, 32, 1])
def test_sim_topk_fp32_bf16_stream_and_prefilter(dev, d, B):
    """sim_topk at d 512 / 1024 (d 1024: the upper limit of the fp32 stream kernel — queries 131 KB of LDS, 120 survivors per workgroup
    — and of the pre-filter): fp32 against float64 scores; the latency mode (B <= 32) against the tiled core (SIM_NO_STREAM); the bf16
    corpus against the oracle on the rounded operands; the pre-filter equal to the all-fp32 path at TOL32."""
    from gdr_amd import ops, _ffi
    from oracle import retrieval_ref
    N, k = 40000, 100
    D = synth.make_corpus(N, d, seed=N + d)
    Q, _ = synth.make_queries(D, B, seed=B)
    Qd, Dd = torch.from_numpy(Q).to(dev), torch.from_numpy(D).to(dev)
    v, i, st = ops.sim_topk(Qd, Dd, k, return_status=True)
    assert int(st.sum()) == 0
    v, i = v.cpu().numpy(), i.cpu().numpy().astype(np.int64)
    rv, ri = _topk64(Q, D, k)
    order_insensitive_topk_match(rv, ri, v, i, TOL)
    assert (np.diff(v, axis=1) <= 0).all()
    if B <= 32:
        v2, i2 = ops.sim_topk(Qd, Dd, k, flags=_ffi.SIM_NO_STREAM)
        order_insensitive_topk_match(v2.cpu().numpy(), i2.cpu().numpy().astype(np.int64), v, i, TOL)
    bv, bi, bs = ops.sim_topk(Qd, ops.to_bf16(Dd), k, return_status=True)
    assert int(bs.sum()) == 0
    qv, qi = retrieval_ref.sim_topk(torch.from_numpy(Q).bfloat16().float(), torch.from_numpy(D).bfloat16().float(), k)
    order_insensitive_topk_match(qv.numpy(), qi.numpy(), bv.cpu().numpy(), bi.cpu().numpy().astype(np.int64), 1e-5)
    pv, pi, ps = ops.sim_topk(Qd, ops.PrefilteredCorpus(Dd), k, return_status=True)
    assert int(ps.sum()) == 0
    order_insensitive_topk_match(v, i, pv.cpu().numpy(), pi.cpu().numpy().astype(np.int64), TOL32)


def test_sim_latency_mode_d1024_degenerate_corpus_is_repaired(dev):
    """60 000 identical docs at d 1024 in latency mode: every doc ties at the threshold, far more than the stream kernel's 120-entry
    survivor list per workgroup.  The default call repairs (status 0) and returns the oracle's answer under the tie rule."""
    from gdr_amd import ops
    d = 1024
    base = synth.make_corpus(8, d, seed=2)
    D = np.repeat(base[:1], 60000, axis=0)
    D[12345] = base[1] * 3.0
    Q, _ = synth.make_queries(base[:2], 3, seed=6)
    Qd, Dd = torch.from_numpy(Q).to(dev), torch.from_numpy(np.ascontiguousarray(D)).to(dev)
    v, i, st = ops.sim_topk(Qd, Dd, 50, return_status=True)
    assert int(st.sum()) == 0
    s = Q.astype(np.float64) @ D.astype(np.float64).T
    for b in range(3):
        order = np.lexsort((np.arange(D.shape[0]), -s[b]))[:50]
        assert np.array_equal(i[b].cpu().numpy(), order), b
        np.testing.assert_allclose(v[b].cpu().numpy(), s[b][order], rtol=TOL, atol=TOL)


@pytest.mark.parametrize("B", [4, 64])
def test_prefilter_adversarial_corpora_at_d1024(dev, B):
    """test_gpu_prefilter's adversarial corpora at d 1024: a near-duplicate cluster (identical bf16 images, fp32 scores 1e-5 apart),
    exact duplicates (lower id first) and coherent bf16 rounding (doc A first in fp32, doc B first by 7 on bf16 operands): the
    pre-filter equals the all-fp32 path, keeps the true top-1, and sets no status."""
    from gdr_amd import ops
    rng = np.random.default_rng(5)
    N, d, k = 50000, 1024, 100
    D = synth.make_corpus(N, d, seed=3)
    near = rng.standard_normal(d).astype(np.float32)
    near /= np.linalg.norm(near)
    where = rng.choice(N, 400, replace=False)
    D[where] = near[None, :] + 1e-5 * rng.standard_normal((400, d)).astype(np.float32)
    dup = rng.standard_normal(d).astype(np.float32)
    dup /= np.linalg.norm(dup)
    where2 = np.setdiff1d(rng.choice(N, 170, replace=False), where)[:150]
    D[where2] = dup[None, :]
    Q = np.stack([near, dup] + [rng.standard_normal(d).astype(np.float32) for _ in range(B - 2)]).astype(np.float32)
    Qd, Dd = torch.from_numpy(Q).to(dev), torch.from_numpy(D).to(dev)
    fv, fi, fs = ops.sim_topk(Qd, Dd, k, return_status=True)
    pv, pi, ps = ops.sim_topk(Qd, ops.PrefilteredCorpus(Dd), k, return_status=True)
    assert int(fs.sum()) == 0 and int(ps.sum()) == 0
    fi, pi = fi.cpu().numpy().astype(np.int64), pi.cpu().numpy().astype(np.int64)
    order_insensitive_topk_match(fv.cpu().numpy(), fi, pv.cpu().numpy(), pi, TOL32)
    assert set(pi[0].tolist()) <= set(where.tolist())
    np.testing.assert_array_equal(pi[1], np.sort(where2)[:k])
    np.testing.assert_array_equal(fi[1], pi[1])
    # coherent rounding: 512 coordinates of 1 + 2^-8 - 2^-14 (bf16 rounds down) against 511 of 1 + 2^-8 + 2^-14 (rounded up)
    lo, hi = np.float32(1 + 2.0 ** -8 - 2.0 ** -14), np.float32(1 + 2.0 ** -8 + 2.0 ** -14)
    D2 = (synth.make_corpus(20000, d, seed=21) * 22.0).astype(np.float32)
    ia, ib = 777, 12345
    D2[ia] = 0
    D2[ia, :512] = lo
    D2[ib] = 0
    D2[ib, 512:1023] = hi
    q = np.zeros(d, np.float32)
    q[:512], q[512:1023] = lo, hi
    Q2 = np.repeat(q[None], B, 0)
    Q2[1::2] *= np.float32(0.5)
    s32 = D2[[ia, ib]].astype(np.float64) @ q.astype(np.float64)
    s16 = (torch.from_numpy(D2[[ia, ib]]).bfloat16().float() @ torch.from_numpy(q).bfloat16().float()).numpy()
    assert s32[0] > s32[1] + 0.8 and s16[1] > s16[0] + 6.0
    Qd, Dd = torch.from_numpy(Q2).to(dev), torch.from_numpy(D2).to(dev)
    for kk in (1, 10):
        fv, fi, fs = ops.sim_topk(Qd, Dd, kk, return_status=True)
        pv, pi, ps = ops.sim_topk(Qd, ops.PrefilteredCorpus(Dd), kk, return_status=True, exact_on_overflow=False)
        assert int(fs.sum()) == 0 and int(ps.sum()) == 0
        assert (fi[:, 0].cpu().numpy() == ia).all() and (pi[:, 0].cpu().numpy() == ia).all()
        order_insensitive_topk_match(fv.cpu().numpy(), fi.cpu().numpy().astype(np.int64), pv.cpu().numpy(),
                                     pi.cpu().numpy().astype(np.int64), 1e-4)


@pytest.mark.parametrize("d", [1032, 1152])
@pytest.mark.parametrize("B", [4, 64])
def test_sim_beyond_d1024_is_served_by_the_tiled_core_or_refused(dev, d, B):
    """Past the stream kernel's and the pre-filter's d <= 1024: either a GdrError or the right answer (the tiled core) — never one of
    those kernels outside its limits."""
    from gdr_amd import ops, _ffi
    N, k = 20000, 50
    D = synth.make_corpus(N, d, seed=d)
    Q, _ = synth.make_queries(D, B, seed=B)
    Qd, Dd = torch.from_numpy(Q).to(dev), torch.from_numpy(D).to(dev)
    rv, ri = _topk64(Q, D, k)
    for corpus in (lambda: Dd, lambda: ops.PrefilteredCorpus(Dd)):
        try:
            v, i, st = ops.sim_topk(Qd, corpus(), k, return_status=True)
        except _ffi.GdrError:
            continue
        assert int(st.sum()) == 0
        order_insensitive_topk_match(rv, ri, v.cpu().numpy(), i.cpu().numpy().astype(np.int64), TOL)


# ------------------------------------------------------------------------------------------- g. doc tower at bert-large widths
def _bert_cfg(hidden, heads, d_ff):
    return dict(vocab_size=30522, hidden_size=hidden, num_heads=heads, d_ff=d_ff, num_layers=2, max_pos=512, type_vocab=2, eps=1e-12)


def test_doc_tower_bert_large_widths_vs_oracle_and_ragged(dev):
    """bert-large widths (hidden 1024, 16 heads, d_ff 4096; 2 layers): padded vs bert_ref at 2e-4, ragged bit-identical to padded."""
    from gdr_amd.modeling import EncoderModel
    from oracle import bert_ref
    bc = _bert_cfg(1024, 16, 4096)
    sd = synth.make_bert_state_dict(bc, seed=77)
    enc = EncoderModel.from_state_dict(bc, sd, dev)
    ids_n, mask_n = synth.make_tokens(24, L=128, vocab_hi=bc["vocab_size"], seed=9, min_len=32)
    ids, mask = torch.from_numpy(ids_n).to(dev), torch.from_numpy(mask_n).to(dev)
    hp, pp = enc.bert.forward(ids, mask, ragged=False)
    sub = slice(0, 6)
    _, ref = bert_ref.bert_forward(sd, bc, torch.from_numpy(ids_n[sub]), torch.from_numpy(mask_n[sub]))
    np.testing.assert_allclose(pp[sub].cpu().numpy(), ref.numpy(), rtol=2e-4, atol=2e-4)
    hr, pr = enc.bert.forward(ids, mask, ragged=True, live_rows_hint=int(mask_n.sum()))
    _, po = enc.bert.forward(ids, mask, ragged=True, want_hidden=False)
    assert torch.equal(pr, pp) and torch.equal(po, pp)
    keep = torch.from_numpy(mask_n != 0).to(dev)
    assert torch.equal(hr[keep], hp[keep]) and int((hr[~keep] != 0).sum()) == 0


@pytest.mark.parametrize("hidden,heads,d_ff", [(1024, 16, 4096), (512, 8, 2048)])
def test_doc_tower_split_form_at_wide_and_narrow_widths(dev, hidden, heads, d_ff):
    """The fp16 x 2 doc tower at 96 passages of 32-128 tokens (>= 8 192 token rows): pooled within 5e-5 of the fp32 form (the base-size
    bound).  hidden 1024: the GeLU epilogue writes wo2's planes (virtual K 3 072); hidden 512: virtual K 1 536 has no plane epilogue,
    so wi stores fp32 and a split launch follows (before the routing fix its plain bf16 image was read as planes)."""
    from gdr_amd.modeling import EncoderModel
    bc = _bert_cfg(hidden, heads, d_ff)
    sd = synth.make_bert_state_dict(bc, seed=78)
    e32 = EncoderModel.from_state_dict(bc, sd, dev, ragged=True)
    esp = EncoderModel.from_state_dict(bc, sd, dev, split=True)
    ids_n, mask_n = synth.make_tokens(96, L=128, vocab_hi=bc["vocab_size"], seed=12, min_len=32)   # 12 288 padded rows: the launcher's M
    ids, mask = torch.from_numpy(ids_n).to(dev), torch.from_numpy(mask_n).to(dev)
    p32 = e32(passage={"input_ids": ids, "attention_mask": mask})
    psp = esp(passage={"input_ids": ids, "attention_mask": mask})
    diff = float((psp - p32).abs().max())
    print(f"fp16 x 2 doc tower hidden {hidden}, 96 passages: max |pooled - fp32 pooled| = {diff:.2e}")
    assert diff <= 5e-5
