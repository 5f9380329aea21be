"""GPU parity of the adaptor-free model (`--adaptor_decode 0 --adaptor_efficient 0`: the docid head is lm_head(sequence_output),
modeling_t5.py:1640-1641) through gdr_t5_generate / gdr_t5_generate_bf16 with the plain form of GdrT5DecoderWeights (csrc/decode.hip
head_plain_kernel): against what the reference itself returned with both flags 0 (g19), bit for bit against the shipped adaptor path
run with adaptor_linear.weight = 0 (0 + e == e: the same head), and against the restatement tests/plain_head_ref.py over the CPU
oracle — beam and greedy, fp32 and bf16, eager and captured, with the trie constraint, through the two-stage step and the CLI."""
import functools
import gc
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import greedy_ref
import plain_head_ref as ph
from conftest import beam_cut_explains_absence, golden, hypothesis_lists_match, ranked_lists_match
from gdr_amd import synth

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _release_the_models_at_the_end():
    yield
    _model.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _model(kind, bf16=False, ragged=False, graph=False, trie=False):
    from gdr_amd import codec
    from gdr_amd.modeling import GDRModel
    cfg = ph.CONFIGS[kind]()
    t = codec.Trie.from_docids(ph.trie_docids(cfg), cfg.output_vocab_size) if trie else None
    return GDRModel(cfg, ph.state_dict(kind), torch.device("cuda:0"), trie=t, ragged=ragged, graph=graph,
                    dtype=torch.bfloat16 if bf16 else torch.float32)


def _close(got, ref, tol=TOL):
    np.testing.assert_allclose(np.asarray(got), np.asarray(ref), rtol=tol, atol=tol)


def _trace_of(model, ids, mask, R, ml, lp):
    enc_h, _ = model.enc.forward(ids, mask, want_pooled=False)
    return model.dec.generate(enc_h, mask, R, ml, lp, R, trace=True, trie=model.trie)


# ------------------------------------------------------------------------------------------------ 1. the reference's own output
@pytest.mark.parametrize("name,tol", [("tiny", 1e-4), ("base", 2e-4)])
def test_generate_vs_reference_golden(dev, name, tol):
    g = golden("g19_generate_plain")
    kind, B, L, R, lp, _ = ph.GOLDEN_BEAM[name]
    model = _model(kind)
    cfg = model.config
    ids = torch.from_numpy(g[f"{name}_input_ids"].astype(np.int64)).to(dev)
    mask = torch.from_numpy(g[f"{name}_attention_mask"].astype(np.int64)).to(dev)
    ref = g[f"{name}_decoded"].astype(np.int64)
    (dec, sc), enc = model.generate(ids, attention_mask=mask, max_length=cfg.max_output_length, num_beams=R, length_penalty=lp,
                                    num_return_sequences=R, output_scores=True, output_encoder_embedding=True)
    assert dec.dtype == torch.int64 and tuple(dec.shape) == ref.shape and isinstance(sc, list) and len(sc) == B * R
    assert np.array_equal(dec.cpu().numpy(), ref)
    print(f"{name}: largest score difference {np.abs(np.array(sc) - g[f'{name}_scores']).max():.3e}")
    _close(sc, g[f"{name}_scores"], tol)
    assert tuple(enc.last_hidden_state.shape) == (B * R, L, cfg.d_model)
    if name == "tiny":
        _close(enc.last_hidden_state[::R].cpu().numpy(), g["tiny_enc"], tol)
    else:
        _close(enc.last_hidden_state[::R, 0].cpu().numpy(), g["base_pooled"], tol)
    dec2, none = model.generate(ids, attention_mask=mask, max_length=cfg.max_output_length, num_beams=R, length_penalty=lp,
                                num_return_sequences=R)
    assert none is None and torch.equal(dec2, dec)
    _, _, _, ts, tt = _trace_of(model, ids, mask, R, cfg.max_output_length, lp)
    ref_s, ref_t = g[f"{name}_step_scores"], g[f"{name}_step_tokens"]
    n = ref_s.shape[0]                                           # the reference stops when every query is done
    live = ref_s > ph.LIVE
    _close(ts.cpu().numpy()[:n][live], ref_s[live], tol)
    assert np.array_equal(tt.cpu().numpy()[:n][live], ref_t[live])


def test_default_generate_call_vs_reference_golden(dev):
    g = golden("g19_generate_plain")
    model = _model(ph.GOLDEN_GREEDY[0])
    ids = torch.from_numpy(g["greedy_input_ids"].astype(np.int64)).to(dev)
    mask = torch.from_numpy(g["greedy_attention_mask"].astype(np.int64)).to(dev)
    ref = torch.from_numpy(g["greedy_ids"].astype(np.int64))
    out, none = model.generate(ids, attention_mask=mask, max_length=int(g["greedy_max_length"]))   # num_beams = 1 by default
    assert none is None and torch.is_tensor(out) and out.dtype == torch.int64 and out.shape == ref.shape
    assert torch.equal(out.cpu(), ref)


# ------------------------------------------------------------------------------------------------ 2. + 3. the shipped path at A = 0
def _handles(kind, dtype):
    from gdr_amd import ops
    d = torch.device("cuda:0")
    plain = ops.T5DecoderHandle(ph.CONFIGS[kind](), ph.state_dict(kind), d, dtype=dtype)
    cfg_a, sd_a = ph.zero_adaptor_twin(kind)
    twin = ops.T5DecoderHandle(cfg_a, sd_a, d, dtype=dtype)
    del sd_a
    assert plain.head_w is None and twin.head_w is not None and int(twin.head_w.float().abs().max()) == 0
    assert torch.equal(plain.head_e, twin.head_e)
    return plain, twin


def _encoder_states(B, L, d, seed, dev):
    g = np.random.Generator(np.random.PCG64(seed))
    enc = torch.from_numpy(g.standard_normal((B, L, d), dtype=np.float32))
    lens = g.integers(1, L + 1, size=B)
    lens[0] = L
    mask = torch.from_numpy((np.arange(L)[None, :] < lens[:, None]).astype(np.int64))
    return enc.to(dev), mask.to(dev)


# kind, B, beams, what the shape reaches
IDENTITY = [
    ("tiny", 3, 4),        # rows * (V+1) = 84 is no multiple of 4; d / 4 = 16 < 64 lanes; step 0's one row per query
    ("tiny_v30", 2, 300),  # 9 300 candidates per query: the chunked select; 600 rows
    ("small2", 2, 6),      # d = 512: two pieces per lane
    ("base2", 2, 10),      # d = 768: three pieces per lane
    ("tiny_v70", 2, 4),    # V + 1 = 71 columns: a second group of 64 columns per row
    ("d256", 2, 3),        # d / 4 == 64: every lane holds exactly one piece
    ("d1024", 2, 3),       # d / 4 == 256: four pieces per lane, the last register form
    ("d1280", 2, 3),       # d / 4 = 320 > 256: the form that reads the row again for every column
]


def _identity(dev, kind, B, R, dtype):
    plain, twin = _handles(kind, dtype)
    cfg = plain.cfg
    ml = cfg.max_output_length
    enc, mask = _encoder_states(B, 7, cfg.d_model, 100 + B * R, dev)
    a = plain.generate(enc, mask, R, ml, 0.8, R, trace=True)
    b = twin.generate(enc, mask, R, ml, 0.8, R, trace=True)
    torch.cuda.synchronize()
    names = ("out_ids", "out_len", "out_scores", "step_scores", "step_tokens")
    assert a[2].dtype == torch.float64 and tuple(a[3].shape) == (ml - 1, B, 2 * R)
    for n, x, y in zip(names, a, b):
        assert torch.equal(x, y), f"{kind} {B} x {R} {dtype}: {n} differs from the adaptor path run with a zero adaptor_linear"
    assert bool(torch.isfinite(a[2]).all()) and int((a[3][-1] > ph.LIVE).sum()) > 0
    # without the trace (the early exit and its gates armed) the same results
    c = plain.generate(enc, mask, R, ml, 0.8, R)
    for n, x, y in zip(names[:3], a, c):
        assert torch.equal(x, y), n
    del plain, twin
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("kind,B,R", IDENTITY, ids=[f"{k}-{b}x{r}" for k, b, r in IDENTITY])
def test_beam_decode_is_bit_identical_to_the_adaptor_path_with_a_zero_adaptor_linear(dev, kind, B, R):
    _identity(dev, kind, B, R, torch.float32)


@pytest.mark.parametrize("kind,B,R", [("tiny8", 3, 4), ("base2", 2, 10)])
def test_bf16_mode_is_bit_identical_to_the_adaptor_path_with_a_zero_adaptor_linear(dev, kind, B, R):
    _identity(dev, kind, B, R, torch.bfloat16)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_greedy_decode_is_identical_to_the_adaptor_path_with_a_zero_adaptor_linear(dev, dtype):
    plain, twin = _handles("tiny8", dtype)
    ml = plain.cfg.max_output_length
    enc, mask = _encoder_states(5, 7, plain.cfg.d_model, 55, dev)
    a = plain.generate(enc, mask, 1, ml, 1.0, 1)
    b = twin.generate(enc, mask, 1, ml, 1.0, 1)
    assert tuple(a[0].shape) == (5, ml) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_bf16_mode_follows_the_emulation(dev):
    """Against the restatement under t5_ref.bf16_linears() (the head dot stays fp32 there too), by the rule of the adaptor path's bf16
    test: scores of shared hypotheses within 5e-3, and ids by oracle/parity_rules.hypothesis_lists_match with that measured gap."""
    from gdr_amd import ops
    from oracle import t5_ref
    cfg, sd, ids, mask, R = ph.case_inputs("bf16")
    B, ml = ids.shape[0], cfg.max_output_length
    model = _model(ph.BF16_CASE[0], bf16=True)
    idt, mt = torch.from_numpy(ids), torch.from_numpy(mask)
    enc_h, _ = model.enc.forward(idt.to(dev), mt.to(dev), want_pooled=False)
    out_ids, lens, scores = model.dec.generate(enc_h, mt.to(dev), R, ml, 0.8, R)
    dec, sc = ops.finish_generate_output(out_ids, lens, scores, ml)
    trace, ptrace = [], []
    with t5_ref.bf16_linears():                               # fed with the GPU's own encoder states: the decode path alone
        (rd, rs), _ = ph.beam_generate(sd, cfg, None, mt, R, trace=trace, prefix_trace=ptrace, enc_hidden=enc_h.cpu())
    sc, rs = np.array(sc).reshape(B, R), np.array(rs).reshape(B, R)
    got, ref = dec.cpu().numpy(), rd.numpy()
    W = min(got.shape[1], ref.shape[1])
    glists = [[tuple(r[:W]) for r in got[b * R:(b + 1) * R].tolist()] for b in range(B)]
    rlists = [[tuple(r[:W]) for r in ref[b * R:(b + 1) * R].tolist()] for b in range(B)]
    gap = 0.0
    for b in range(B):
        where = {x: i for i, x in enumerate(rlists[b])}
        gap = max([gap] + [abs(sc[b, p] - rs[b, where[x]]) for p, x in enumerate(glists[b]) if x in where])
    print(f"bf16 plain head: hypothesis scores of the GPU and the emulation differ by at most {gap:.2e} (bound {ph.BF16_BOUND:g})")
    assert gap <= ph.BF16_BOUND
    tie = max(gap, 2e-4)
    shared = 0
    for b in range(B):
        def explain(hyp, b=b):
            return beam_cut_explains_absence(trace, ptrace, b, R, cfg.decode_vocab_size, list(hyp), tie, final_cut=rs[b, -1])
        hypothesis_lists_match(rlists[b], rs[b], glists[b], tie, explain_foreign=explain)
        shared += len(set(glists[b]) & set(rlists[b]))
    assert shared >= 0.8 * B * R, (shared, B * R)


# ------------------------------------------------------------------------------------------------ 4. the restatement
def _check_against_the_restatement(dev, name, model):
    (rd, rs), trace, _, renc, gap = ph.oracle(name)
    print(f"{name}: smallest gap of the restatement {gap:.3e} (need >= {ph.GAP:g})")
    assert gap >= ph.GAP
    cfg, _, ids, mask, R = ph.case_inputs(name)
    idt, mt = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)
    (dec, sc), enc = model.generate(idt, attention_mask=mt, max_length=cfg.max_output_length, num_beams=R, length_penalty=0.8,
                                    num_return_sequences=R, output_scores=True, output_encoder_embedding=True)
    assert np.array_equal(dec.cpu().numpy(), rd.numpy())
    rs = np.array(rs)
    fin = np.isfinite(rs)
    _close(np.array(sc)[fin], rs[fin])
    assert np.array_equal(np.isfinite(np.array(sc)), fin)
    keep = mask.astype(bool)
    _close(enc.last_hidden_state[::R].cpu().numpy()[keep], renc.numpy()[keep])
    _, _, _, ts, tt = _trace_of(model, idt, mt, R, cfg.max_output_length, 0.8)
    ts, tt = ts.cpu().numpy(), tt.cpu().numpy()
    for s, (ref_s, ref_t) in enumerate(trace):
        live = ref_s.numpy() > ph.LIVE
        _close(ts[s][live], ref_s.numpy()[live])
        assert np.array_equal(tt[s][live], ref_t.numpy()[live]), (name, s)


@pytest.mark.parametrize("name", ["b1_r2_l3", "b5_r6_l9", "b2_r16_l12"])
def test_beam_decode_vs_the_restatement(dev, name):
    _check_against_the_restatement(dev, name, _model("tiny"))


def test_long_input_takes_the_key_block_cross_attention(dev):
    _check_against_the_restatement(dev, "l200", _model("tiny"))                 # L = 200 > 128 keys


def test_ragged_encoder_feeds_the_plain_head(dev):
    _check_against_the_restatement(dev, "ragged", _model("tiny", ragged=True))


def test_trie_constraint_vs_the_restatement_with_decode_tree(dev):
    model = _model("tiny", trie=True)
    _check_against_the_restatement(dev, "trie", model)
    cfg, _, ids, mask, R = ph.case_inputs("trie")
    dec, _ = model.generate(torch.from_numpy(ids).to(dev), attention_mask=torch.from_numpy(mask).to(dev),
                            max_length=cfg.max_output_length, num_beams=R, length_penalty=0.8, num_return_sequences=R)
    docs = {tuple(ph.docid_tokens(n, cfg.output_vocab_size)) for n in ph.trie_docids(cfg)}
    rows = [tuple(t for t in r[1:] if t != 0) for r in dec.cpu().tolist()]
    assert sum(r in docs for r in rows) >= len(rows) // 2          # the constraint steers the beams onto docids of the trie
    free, _ = _model("tiny").generate(torch.from_numpy(ids).to(dev), attention_mask=torch.from_numpy(mask).to(dev),
                                      max_length=cfg.max_output_length, num_beams=R, length_penalty=0.8, num_return_sequences=R)
    assert free.shape != dec.shape or not torch.equal(free, dec)   # ... which the unconstrained search does not return


# ------------------------------------------------------------------------------------------------ 5. graph capture, early exit
def test_graph_replay_equals_the_eager_call(dev):
    cfg, _, ids, mask, R = ph.case_inputs("b5_r6_l9")
    idt, mt = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)
    kw = dict(attention_mask=mt, max_length=cfg.max_output_length, num_beams=R, length_penalty=0.8, num_return_sequences=R,
              output_scores=True)
    (dec, sc), _ = _model("tiny").generate(idt, **kw)
    eager_greedy, _ = _model("tiny").generate(idt, attention_mask=mt, max_length=cfg.max_output_length)
    graphed = _model("tiny", graph=True)
    for _ in range(3):                                           # captured, then replayed twice
        (d2, s2), _ = graphed.generate(idt, **kw)
        assert torch.equal(d2, dec) and s2 == sc
        g2, _ = graphed.generate(idt, attention_mask=mt, max_length=cfg.max_output_length)
        assert torch.equal(g2, eager_greedy)
    assert np.array_equal(dec.cpu().numpy(), ph.oracle("b5_r6_l9")[0][0].numpy())


CHILD = r"""
import json, sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import greedy_ref, plain_head_ref as ph
from gdr_amd import _ffi, ops
torch.set_grad_enabled(False)
dev = torch.device("cuda:0")
cfg, sd, T, Q = greedy_ref.crafted()                      # lm_head is a small-integer table: EOS wins where the program says
sd = {k: v for k, v in sd.items() if not k.startswith("adaptor")}
handle = ops.T5DecoderHandle(ph.tiny(), sd, dev)
out = {}
hexed = lambda t: t.cpu().numpy().tobytes().hex()
groups = [3, 4, 3, 4, 3]                                  # every row emits EOS as its second token
enc, mask = greedy_ref.crafted_encoder_rows(groups, cfg.d_model, cfg.decode_vocab_size)
for R in (2, 1):
    for rep in range(3):
        ids, lens, scores = handle.generate(enc.to(dev), mask.to(dev), R, greedy_ref.CRAFTED_MAX_LENGTH, 1.0, R)
    out[str(R)] = {"ids": hexed(ids), "len": hexed(lens), "scores": hexed(scores), "width": int(lens.max())}
torch.cuda.synchronize()
out["early_exits"] = int(_ffi.lib().gdr_t5_generate_early_exits())
out["last_done_step"] = int(_ffi.lib().gdr_t5_generate_last_done_step())     # of the greedy call just above
print("RESULT " + json.dumps(out))
"""


def _run(**env):
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])


def test_leaving_the_step_loop_early_changes_no_byte():
    base, full = _run(), _run(GDR_DECODE_EARLY_EXIT="0")
    base.pop("early_exits")                                   # the host half races with the GPU by design: not asserted
    done = base.pop("last_done_step")
    assert 0 < done < greedy_ref.CRAFTED_MAX_LENGTH and done == 2 and base["1"]["width"] == 3
    assert full.pop("early_exits") == 0 and full.pop("last_done_step") == 0
    assert full == base, "out_ids, out_len and out_scores must be byte-identical with and without the early exit"


# ------------------------------------------------------------------------------------------------ 6. the two-stage step
STAGE2 = dict(B=4, R=4, L=10, docs=600, csz=12, seed=1)


def _stage2_inputs():
    from gdr_amd import codec
    cfg = ph.tiny()
    V = cfg.output_vocab_size
    names, depth, offs, members = synth.make_cluster_ids(STAGE2["docs"], cluster_size=STAGE2["csz"], V=V)
    assert depth + 2 <= cfg.max_output_length
    D = synth.make_corpus(STAGE2["docs"], cfg.d_model, cluster_size=STAGE2["csz"], seed=8)
    ids, mask = synth.make_tokens(STAGE2["B"], L=STAGE2["L"], vocab_hi=cfg.vocab_size, seed=STAGE2["seed"], min_len=3)
    args = types.SimpleNamespace(num_return_sequences=STAGE2["R"], output_vocab_size=V, max_output_length=cfg.max_output_length,
                                 length_penalty=0.8, kary=V, position=1, score_rate=[0, 0.5, 2.0], loss_func="tanh")
    return cfg, codec.ClusterIndex(names, offs, members), D, ids, mask, args


def _stage2_reference(cfg, index, D, ids, mask, args):
    """oracle.retrieval_ref fed with the restatement's decoded rows and scores: per query and alpha (values, doc ids)."""
    from gdr_amd import codec
    from oracle import retrieval_ref
    R = args.num_return_sequences
    from oracle import beam_ref
    tree = beam_ref.build_trie([ph.docid_tokens(n, cfg.output_vocab_size) for n in index.names])
    trace = []
    (rd, rs), enc = ph.beam_generate(ph.state_dict("tiny"), cfg, torch.from_numpy(ids), torch.from_numpy(mask), R,
                                     max_length=args.max_output_length, length_penalty=args.length_penalty, decode_tree=tree,
                                     trace=trace)
    gap = ph.beam_min_gap([s.numpy() for s, _ in trace], rs, ids.shape[0], R)
    print(f"two-stage step: smallest gap of the restatement {gap:.3e} (need >= {ph.GAP:g})")
    assert gap >= ph.GAP
    dec = codec.dec_2d(codec.decode_token(args, rd.numpy()), R)
    q = enc[:, 0]
    bs = np.array(rs, np.float32).reshape(-1, R)
    out = []
    for b in range(ids.shape[0]):
        mem = [m for s_ in dec[b] for m in index[s_]]
        num = [len(index[s_]) for s_ in dec[b]]
        out.append(retrieval_ref.rerank(q[b:b + 1], torch.from_numpy(D), [mem], [num], bs[b:b + 1].tolist(), args.score_rate,
                                        min(R, len(mem)))[0] if mem else None)
    return dec, out


def test_two_stage_step_with_the_plain_model(dev):
    """The corpus' docids constrain the search (trie=, as `--constrain_tree 1` does): unconstrained random weights rarely spell the
    id of one of the 50 clusters, and stage 2 would have nothing to rank."""
    from gdr_amd import codec
    from gdr_amd.modeling import GDRModel, GDRRetriever
    cfg, index, D, ids, mask, args = _stage2_inputs()
    R = args.num_return_sequences
    dec, ref = _stage2_reference(cfg, index, D, ids, mask, args)
    model = GDRModel(cfg, ph.state_dict("tiny"), dev, trie=codec.Trie.from_docids(index.names, cfg.output_vocab_size))
    retr = GDRRetriever(model, torch.from_numpy(D).to(dev), index, args)
    out = retr.validation_step_i({"source_ids": torch.from_numpy(ids).to(dev), "source_mask": torch.from_numpy(mask).to(dev)})
    assert [list(x) for x in out["clusters"]] == [list(x) for x in dec]
    vals, idx = out["rerank_values"].cpu().numpy(), out["doc_id_tensor"].cpu().numpy()
    assert all(r is not None for r in ref), "the decoded clusters must name documents for the step to rerank"
    for b, per_alpha in enumerate(ref):
        if per_alpha is None:
            assert (idx[b] == -1).all()
            continue
        for a in range(len(args.score_rate)):
            rv, ri = per_alpha[a]
            kk = rv.numel()
            np.testing.assert_allclose(vals[b, a, :kk], rv.numpy(), rtol=TOL, atol=TOL)
            ranked_lists_match(ri.tolist(), rv.numpy(), idx[b, a, :kk].tolist(), TOL)
            assert (idx[b, a, kk:] == -1).all()


# ------------------------------------------------------------------------------------------------ 7. the command line
CLI = dict(n_queries=4, L=11, R=4, ml=4, docs=600)     # L: the first of 12, 10, 14, 16, 9, 11 at which the restatement clears GAP


def test_cli_eval_with_the_flag_pair_writes_the_restatement_s_res1(dev, tmp_path):
    """`--mode eval --adaptor_decode 0 --adaptor_efficient 0` on the synthetic workload at the smallest model the CLI names
    (--model_info small): res1 holds, per query, the clusters the restatement decodes."""
    from gdr_amd import codec, main as gmain
    path = tmp_path / "res1.tsv"
    argv = ["--mode", "eval", "--adaptor_decode", "0", "--adaptor_efficient", "0", "--prefix_table", "0", "--model_info", "small",
            "--corpus_rows", str(CLI["docs"]), "--n_queries", str(CLI["n_queries"]), "--max_input_length", str(CLI["L"]),
            "--num_return_sequences", str(CLI["R"]), "--eval_batch_size", "4", "--max_output_length", str(CLI["ml"]),
            "--score_rate", "0", "1", "--res1_save_path", str(path)]
    gmain.main(argv)
    args = gmain.parsers_parser(argv)
    cfg = ph.GDRConfig.from_args(args)
    assert not cfg.has_adaptor
    sd = synth.make_state_dict(cfg, seed=1234)
    ids, mask = synth.make_tokens(CLI["n_queries"], L=CLI["L"], seed=11)
    trace = []
    (rd, rs), _ = ph.beam_generate(sd, cfg, torch.from_numpy(ids), torch.from_numpy(mask), CLI["R"], max_length=CLI["ml"],
                                   length_penalty=args.length_penalty, trace=trace)
    gap = ph.beam_min_gap([s.numpy() for s, _ in trace], rs, CLI["n_queries"], CLI["R"])
    print(f"cli: smallest gap of the restatement {gap:.3e} (need >= {ph.GAP:g})")
    assert gap >= ph.GAP
    dec = codec.dec_2d(codec.decode_token(args, rd.numpy()), CLI["R"])
    names = synth.make_cluster_ids(CLI["docs"], cluster_size=12, V=args.kary)[0]
    gold = synth.make_gold(CLI["docs"], CLI["n_queries"])
    want = sorted(["q%d" % b, ",".join(dec[b]), names[int(gold[b]) // 12], "1"] for b in range(CLI["n_queries"]))
    got = [ln.rstrip("\n").split("\t") for ln in open(path)]
    assert got[:CLI["n_queries"]] == want
