"""The beam decode beyond 256 beams and beyond 8192 candidates per query and step (csrc/beam.hip: beam_topk_kernel up to 8192
keys, above that beam_norm_kernel / beam_chunk_kernel / sel_merge_kernel — the same top-2R list bit for bit), up to 1024 beams,
through gdr_beam_search_table, gdr_t5_generate and the two-stage retriever.  Semantics: generation_utils.py:629-921.

The parity rule against the float64 oracle (exact row order cannot be asked for: adjacent final float64 scores lie as close
as 2.7e-7 at these widths and the GPU's expf / logf round differently): _check_query below, tolerance 1e-5 throughout."""
import functools
import hashlib
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from conftest import beam_cut_explains_absence, order_insensitive_topk_match
from gdr_amd import synth
from gdr_amd.config import GDRConfig

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL, LP = 1e-5, 0.8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------ the rule
def _canon(row):
    """START, tokens, [EOS], PAD ... -> the tuple without its padding (PAD = START = 0; every other token is > 0)."""
    row = [int(t) for t in row]
    while len(row) > 1 and row[-1] == 0:
        row.pop()
    return tuple(row)


def _near_a_cut(trace, ptrace, q, R, Vd, row, tol):
    """A row of the ORACLE's list that the other list lacks: legitimate only if its score is within tol of the oracle's last
    returned score (the caller looks), or if at some step its candidate sat within tol (on the final-score scale) of that step's cut — the first
    non-EOS candidate that was not continued, or for its EOS candidate the rank-R candidate."""
    toks = list(row)
    ended = 1 in toks[1:]
    if ended:
        toks = toks[:1 + toks[1:].index(1)]
    n = len(toks) - 1
    for s in range(min(n + 1, len(trace))):
        sc, tk = trace[s][0][q].tolist(), trace[s][1][q].tolist()
        pref = ptrace[s][q * R:(q + 1) * R].tolist()
        if toks[:s + 1] not in pref:
            return None
        want = pref.index(toks[:s + 1]) * Vd + (toks[s + 1] if s < n else 1)
        if want not in tk:
            return None
        r = tk.index(want)
        tol_s = tol * float(s + 1) ** LP
        if s == n:
            return f"EOS candidate ties rank {R} at step {s}" if r < R and abs(sc[r] - sc[R]) <= tol_s else None
        non_eos = [i for i, t in enumerate(tk) if t % Vd != 1]
        if len(non_eos) > R and abs(sc[r] - sc[non_eos[R]]) <= tol_s:
            return f"ties the first pruned candidate of step {s}"
    return None


def _check_query(ref_rows, ref_sc, got_rows, got_sc, trace, ptrace, q, R, Vd, tol=TOL):
    """ref_rows / got_rows: the query's hypotheses in returned order (canonical tuples), scores beside them.
      * sorted scores agree within rtol = atol = tol;
      * the oracle's list is cut into maximal runs of adjacent scores closer than tol: rows that both lists hold keep the order
        of the runs (inside a run any permutation);
      * a row in one list only: its oracle score lies within tol of the oracle's last returned score or of a step's cut;
      * at most 5 % of the rows sit at another rank than the oracle's.
    Returns (run sizes, moved, one-sided rows)."""
    k = len(ref_rows)
    assert len(got_rows) == k and len(set(ref_rows)) == k and len(set(got_rows)) == k
    ref_sc, got_sc = np.asarray(ref_sc, np.float64), np.asarray(got_sc, np.float64)
    np.testing.assert_allclose(np.sort(got_sc)[::-1], np.sort(ref_sc)[::-1], rtol=tol, atol=tol)
    run, sizes = np.zeros(k, np.int64), [1]
    for i in range(1, k):
        if ref_sc[i - 1] == ref_sc[i] or abs(ref_sc[i - 1] - ref_sc[i]) < tol:
            run[i] = run[i - 1]
            sizes[-1] += 1
        else:
            run[i] = run[i - 1] + 1
            sizes.append(1)
    pos = {x: i for i, x in enumerate(ref_rows)}
    moved, last_run, one_sided = 0, -1, 0
    for p, x in enumerate(got_rows):
        r = pos.get(x)
        if r is None:
            why = beam_cut_explains_absence(trace, ptrace, q, R, Vd, list(x), tol / 2, lp=LP, final_cut=float(ref_sc[-1]))
            assert why, ("a row outside the oracle's list that no cut of the oracle's search explains by a tie", q, p, x, got_sc[p])
            one_sided += 1
            continue
        assert run[r] >= last_run, ("two rows swapped across runs of the oracle's list", q, p, r, ref_sc[r])
        last_run = run[r]
        moved += int(r != p)
    have = set(got_rows)
    for i, x in enumerate(ref_rows):
        if x not in have:
            why = "ties the last returned score" if abs(ref_sc[i] - ref_sc[-1]) <= tol else \
                _near_a_cut(trace, ptrace, q, R, Vd, x, tol)
            assert why, ("a row of the oracle's list is missing and sits at no cut", q, i, x, ref_sc[i])
            one_sided += 1
    assert moved <= 0.05 * k, (q, moved, k)
    return sizes, moved, one_sided


def _check_lists(ref_dec, ref_sc, got_dec, got_sc, trace, ptrace, B, R, nret, Vd, label, tol=TOL):
    ref_rows, got_rows = [_canon(r) for r in ref_dec.tolist()], [_canon(r) for r in got_dec.tolist()]
    ref_sc, got_sc = np.asarray(ref_sc, np.float64).reshape(B, nret), np.asarray(got_sc, np.float64).reshape(B, nret)
    for q in range(B):
        sizes, moved, one = _check_query(ref_rows[q * nret:(q + 1) * nret], ref_sc[q], got_rows[q * nret:(q + 1) * nret], got_sc[q],
                                         trace, ptrace, q, R, Vd, tol)
        big = sorted((s for s in sizes if s > 1), reverse=True)
        print(f"{label} query {q}: {len(sizes)} runs over {nret} rows, {len(big)} of more than one row {big[:8]}, "
              f"{moved} rows at another rank, {one} one-sided")


# ------------------------------------------------------------------------------------------ table-driven: oracle, once per shape
@functools.lru_cache(maxsize=None)
def _table_oracle(V, maxlen, R, B, boost, seed, nret=None, n_docids=0):
    """The float64 oracle on synth.make_logit_table; with n_docids a trie over that many random docids of depth maxlen - 1."""
    from oracle import beam_ref, t5_ref
    Vd = V * maxlen + 2
    tab = synth.make_logit_table(B, maxlen, Vd, boost, seed)
    table = torch.from_numpy(tab).double()
    qid = torch.arange(B).repeat_interleave(R)
    tree = docids = None
    if n_docids:
        rng = np.random.default_rng(seed)
        docids = sorted({tuple(int(x) for x in rng.integers(0, V, maxlen - 1)) for _ in range(n_docids)})
        tree = beam_ref.build_trie([[p * V + 2 + c for p, c in enumerate(dd)] + [1] for dd in docids])

    def step(seq):
        t = seq.shape[1]
        return table[qid, t - 1, seq[:, -1]] + t5_ref.positional_mask(t, Vd, V)[t - 1].double()

    trace, ptrace = [], []
    dec, sc = beam_ref.beam_search(step, B, R, Vd, maxlen, LP, nret, trace=trace, decode_tree=tree, prefix_trace=ptrace)
    return tab, dec.numpy(), np.array(sc), trace, ptrace, docids


def _table_case(dev, V, maxlen, R, B, boost, seed, nret=None, n_docids=0):
    from gdr_amd import codec, ops
    tab, ref_dec, ref_sc, trace, ptrace, docids = _table_oracle(V, maxlen, R, B, boost, seed, nret, n_docids)
    trie = None
    if docids:
        trie = ops.DeviceTrie(codec.Trie.from_docids(["-".join(str(c) for c in dd) for dd in docids], V), dev)
        assert np.isfinite(ref_sc).all(), "the trie must hold enough docids for every returned row to be one"
    ids, lens, scores = ops.beam_search_table(torch.from_numpy(tab).to(dev), V, R, maxlen, LP, nret, trie=trie)
    dec, sc = ops.finish_generate_output(ids, lens, scores, maxlen)
    _check_lists(ref_dec, ref_sc, dec.cpu().numpy(), sc, trace, ptrace, B, R, nret or R, V * maxlen + 2,
                 f"table V={V} R={R} ml={maxlen}")
    return ref_dec


WIDE = [(40, 4, 256, 2, 3.0, 5),      # 10 496 candidates: the sort limit alone
        (30, 5, 300, 2, 4.0, 9),      # both limits
        (30, 5, 1024, 1, 4.0, 13),    # 31 744 candidates
        (6, 5, 1024, 1, 2.5, 17),     # the beam limit alone (one-sort form); hypotheses end early: the heap's add / evict paths
        (63, 4, 1024, 1, 3.0, 21)]    # 65 536 candidates


@pytest.mark.parametrize("V,maxlen,R,B,boost,seed", WIDE)
def test_beam_search_beyond_the_old_limits_vs_float64_oracle(dev, V, maxlen, R, B, boost, seed):
    ref_dec = _table_case(dev, V, maxlen, R, B, boost, seed)
    if V == 6:
        early = sum(1 for row in ref_dec.tolist() if 1 in row[1:-1])
        assert early >= 20, f"want hypotheses that ended early, have {early}"


def test_beam_search_300_beams_returning_10(dev):
    _table_case(dev, 30, 5, 300, 2, 4.0, 9, nret=10)


def test_beam_search_300_beams_inside_a_trie(dev):
    _table_case(dev, 30, 5, 300, 2, 4.0, 9, n_docids=400)


@pytest.mark.parametrize("V,maxlen,R,B,boost,seed", [
    (31, 4, 257, 2, 3.0, 25),     # 8 224 candidates: the smallest chunked call (3 chunks, 32 live keys in the last)
    (32, 4, 250, 1, 3.0, 29),     # 8 250 candidates: the last chunk holds 58 live keys, fewer than 2R = 500
    (16, 4, 1000, 1, 3.0, 33)])   # 17 000 candidates: five chunks (616 live keys in the last, 2R = 2000), two merge rounds
def test_chunk_edges_vs_float64_oracle(dev, V, maxlen, R, B, boost, seed):
    n = R * (V + 1)
    assert n > 8192 and 0 < n % 4096 < 2 * R
    _table_case(dev, V, maxlen, R, B, boost, seed)


# ------------------------------------------------------------------------------------------ the model path
MODEL_TOL = 1e-4   # the model tests' tolerance (tests/test_gpu_decode.py): the HIP path's logits differ from the oracle's by fp32
                   # summation order, which the table-driven cases above do not have


@functools.lru_cache(maxsize=None)
def _tiny_oracle(B, R, L):
    """beam_ref.generate(..., restricted_head=True) spelled out, so that the search also leaves its prefix trace."""
    from oracle import beam_ref, t5_ref
    cfg = GDRConfig.tiny()
    sd = synth.make_state_dict(cfg, seed=99)
    ids, mask = synth.make_tokens(B, L=L, vocab_hi=cfg.vocab_size, seed=B + R, min_len=1)
    it, mt = torch.from_numpy(ids), torch.from_numpy(mask)
    enc = t5_ref.encoder_forward(sd, cfg, it, mt)
    idx = torch.arange(B).view(-1, 1).repeat(1, R).view(-1)
    enc_x, mask_x = enc.index_select(0, idx), mt.index_select(0, idx)
    trace, ptrace = [], []
    rd, rs = beam_ref.beam_search(lambda seq: t5_ref.decode_logits(sd, cfg, seq, enc_x, mask_x, restricted=True), B, R,
                                  cfg.decode_vocab_size, cfg.max_output_length, LP, R, cfg.eos_token_id, cfg.pad_token_id,
                                  cfg.decoder_start_token_id, trace=trace, prefix_trace=ptrace)
    return cfg, sd, ids, mask, enc, rd.numpy(), np.array(rs), trace, ptrace


@pytest.mark.parametrize("with_table", [False, True], ids=["computed", "prefix_table"])
def test_generate_tiny_300_beams_vs_oracle(dev, with_table):
    """generate() of the tiny model at B = 2, R = 300, L = 9 (2 100 candidates: the beam limit alone) against the fp32 oracle,
    with the head computed for every row and with a prefix table that has holes (hit and miss rows share a step)."""
    from gdr_amd import codec
    from gdr_amd.modeling import GDRModel
    B, R, L = 2, 300, 9
    cfg, sd, ids, mask, _enc, rd, rs, trace, ptrace = _tiny_oracle(B, R, L)
    assert np.isfinite(rs).all()
    V = cfg.output_vocab_size
    trie = codec.Trie.from_docids([f"{a}-{b}" for a in range(V) for b in range(V) if (a * V + b) % 3], V) if with_table else None
    model = GDRModel(cfg, sd, dev, prefix_trie=trie)
    (dec, sc), _ = model.generate(torch.from_numpy(ids).to(dev), attention_mask=torch.from_numpy(mask).to(dev),
                                  max_length=cfg.max_output_length, num_beams=R, length_penalty=LP, num_return_sequences=R,
                                  output_scores=True)
    _check_lists(rd, rs, dec.cpu().numpy(), sc, trace, ptrace, B, R, R, cfg.decode_vocab_size,
                 f"generate R={R} table={with_table}", MODEL_TOL)


def test_two_stage_retrieval_at_300_beams_vs_oracle(dev):
    """validation_step_i at R = 300 on the tiny model: decode -> id_mapping -> rerank (k = R) against the oracle composition of
    the same stages (tests/test_gpu_decode.py test_two_stage_retrieval_vs_oracle), the cluster index built from the strings the
    oracle decode produces plus fillers.  Stage 1 under the hypothesis rule at the model tolerance, stage 2 under the
    tie-tolerant top-k rule."""
    from gdr_amd import codec
    from gdr_amd.modeling import GDRModel, GDRRetriever
    from oracle import codec_ref, retrieval_ref
    B, R, L, csize = 2, 300, 9, 2
    cfg, sd, ids, mask, enc, rd, rs, trace, ptrace = _tiny_oracle(B, R, L)
    V = cfg.output_vocab_size
    dec = codec_ref.dec_2d(codec_ref.decode_token(rd, output_vocab_size=V, kary=V), R)
    names = [f"filler-{i}" for i in range(5)] + sorted({s for row in dec for s in row}) + [f"filler-{i}" for i in range(5, 9)]
    N = len(names) * csize
    offsets = (np.arange(len(names) + 1) * csize).astype(np.int32)
    members = np.random.Generator(np.random.PCG64(3)).permutation(N).astype(np.int32)
    D = synth.make_corpus(N, cfg.d_model, cluster_size=csize, seed=8)
    args = types.SimpleNamespace(num_return_sequences=R, output_vocab_size=V, max_output_length=cfg.max_output_length,
                                 length_penalty=LP, kary=V, position=1, score_rate=[0, 1.0], loss_func="tanh")
    retr = GDRRetriever(GDRModel(cfg, sd, dev), torch.from_numpy(D).to(dev), codec.ClusterIndex(names, offsets, members), args)
    out = retr.validation_step_i({"source_ids": torch.from_numpy(ids).to(dev), "source_mask": torch.from_numpy(mask).to(dev)})
    got_sc, ref_sc = np.array(out["inf_result_batch_prob"]).reshape(B, R), rs.reshape(B, R)
    for q in range(B):
        assert len(set(dec[q])) == R                 # distinct hypotheses decode to distinct cluster strings: compare as rows
        ref_rows = [_canon(r) for r in rd[q * R:(q + 1) * R].tolist()]
        by_name = dict(zip(dec[q], ref_rows))
        got_rows = [by_name.get(s, ("not in the oracle's list", s)) for s in out["clusters"][q]]
        sizes, moved, one = _check_query(ref_rows, ref_sc[q], got_rows, got_sc[q], trace, ptrace, q, R, cfg.decode_vocab_size, MODEL_TOL)
        print(f"two-stage query {q}: {len(sizes)} runs, {moved} rows at another rank, {one} one-sided")
    look = {n: i for i, n in enumerate(names)}
    mem_q = [[m for s in row for m in members[offsets[look[s]]:offsets[look[s] + 1]].tolist()] for row in dec]
    num_q = [[csize for _ in row] for row in dec]
    ref = retrieval_ref.rerank(enc[:, 0], torch.from_numpy(D), mem_q, num_q, ref_sc.astype(np.float32).tolist(), args.score_rate, R)
    for b in range(B):
        for a in range(len(args.score_rate)):
            order_insensitive_topk_match(ref[b][a][0].numpy()[None], ref[b][a][1].numpy()[None],
                                         out["rerank_values"][b, a].cpu().numpy()[None],
                                         out["doc_id_tensor"][b, a].cpu().numpy().astype(np.int64)[None], MODEL_TOL)


# ------------------------------------------------------------------------------------------ forced chunked form == one-sort form
CHILD = r"""
import hashlib, json, sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
from gdr_amd import codec, ops, synth
from gdr_amd.config import GDRConfig
from gdr_amd.modeling import GDRModel
torch.set_grad_enabled(False)
dev = torch.device("cuda:0")

def digest(*ts):
    h = hashlib.sha256()
    for t in ts:
        h.update(np.ascontiguousarray(t.cpu().numpy()).tobytes())
    return h.hexdigest()

out = {}
for V, R in ((30, 100), (12, 100), (6, 6), (31, 256)):
    ml, B = 4, 2
    tab = torch.from_numpy(synth.make_logit_table(B, ml, V * ml + 2, 3.0, 40 + V)).to(dev)
    out[f"table_{V}x{R}"] = digest(*ops.beam_search_table(tab, V, R, ml, 0.8))
cfg = GDRConfig.tiny()
sd = synth.make_state_dict(cfg, seed=1234)
V, ml = cfg.output_vocab_size, cfg.max_output_length
ids, mask = synth.make_tokens(5, L=9, vocab_hi=cfg.vocab_size, seed=4, min_len=2)
it, mt = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)
holes = codec.Trie.from_docids([f"{a}-{b}" for a in range(V) for b in range(V) if (a * V + b) % 3], V)
for name, kw in (("plain", {}), ("trie", dict(trie=holes)), ("prefix_table", dict(prefix_trie=holes)),
                 ("bf16", dict(dtype=torch.bfloat16)), ("bf16_table", dict(dtype=torch.bfloat16, prefix_trie=holes))):
    m = GDRModel(cfg, sd, dev, **kw)
    enc_h, _ = m.enc.forward(it, mt, want_pooled=False)
    for R in (6, 16):
        out[f"{name}_R{R}"] = digest(*m.dec.generate(enc_h, mt, R, ml, 0.8, R, trace=True, trie=m.trie, prefix_table=m.prefix_table))
# no trace, so the early exit and its device-side gate are on.  max_length = 6; B = 5, R = 16 inside a trie in which ONE query is done
# a step before the end (the test beside this one shows it on the oracle): it pads while the others go on ...
cfg6 = GDRConfig.tiny(max_output_length=6)
sd6 = synth.make_state_dict(cfg6, seed=1234)
ids, mask = synth.make_tokens(5, L=9, vocab_hi=cfg6.vocab_size, seed=5, min_len=2)
it, mt = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)
m = GDRModel(cfg6, sd6, dev, trie=codec.Trie.from_docids(json.loads(sys.argv[2]), V))
enc_h, _ = m.enc.forward(it, mt, want_pooled=False)
out["early_one_R16"] = digest(*m.dec.generate(enc_h, mt, 16, 6, 0.8, 16, trie=m.trie))
# ... and inside a trie of one-digit docids EVERY query is done two steps before the end: the launches behind it exit at the gate
m = GDRModel(cfg6, sd6, dev, trie=codec.Trie.from_docids([str(a) for a in range(V)], V))
out["early_all_R6"] = digest(*m.dec.generate(enc_h, mt, 6, 6, 0.8, 6, trie=m.trie))
torch.cuda.synchronize()
from gdr_amd import _ffi
out["last_done_step"] = int(_ffi.lib().gdr_t5_generate_last_done_step())
print("RESULT " + json.dumps(out))
"""


def _early_docids(V):
    """Two-digit docids under the digits 0, 2, 4 (their beams may only emit EOS at step 2) and two four-digit docids under 1: a
    query whose 16 beams of step 2 hold neither deep prefix fills its heap there and is done a step later; the others are not."""
    return [f"{a}-{b}" for a in (0, 2, 4) for b in range(V)] + ["1-0-0-0", "1-1-1-1"]


def test_forced_chunked_select_is_bit_identical_to_the_one_sort_form():
    """GDR_DECODE_BEAM_CHUNKED=1 sends every select through the norm / chunk / merge kernels: ids, lengths, fp64 scores and the
    per-step top-2R trace must keep every bit.  The switch is read once per process: one fresh child per setting."""
    cfg = GDRConfig.tiny()
    docids = _early_docids(cfg.output_vocab_size)
    res = {}
    for v in ("0", "1"):
        r = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps(docids)], env=dict(os.environ, GDR_DECODE_BEAM_CHUNKED=v),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (v, r.returncode, r.stderr[-2000:])        # a faulted or timed-out child ends the test here
        res[v] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    assert res["0"].keys() == res["1"].keys() and len(res["0"]) == 4 + 10 + 3
    diff = [k for k in res["0"] if res["0"][k] != res["1"][k]]
    assert not diff, diff
    # the last call (one-digit docids) ended before max_length in both forms: every query done, the device-side gate closed
    assert 0 < res["0"]["last_done_step"] < 5, res["0"]["last_done_step"]


def test_one_query_of_the_early_exit_case_is_done_before_the_others():
    """The precondition of the digest `early_one_R16` above, on the CPU oracle: inside _early_docids' trie exactly the queries
    whose beams dropped both deep prefixes are done (BeamHypotheses.is_done) before the last step, the others never."""
    from oracle import beam_ref, codec_ref
    cfg = GDRConfig.tiny(max_output_length=6)
    sd = synth.make_state_dict(cfg, seed=1234)
    V = cfg.output_vocab_size
    ids, mask = synth.make_tokens(5, L=9, vocab_hi=cfg.vocab_size, seed=5, min_len=2)
    tree = beam_ref.build_trie([codec_ref.encode_single_newid(s, kary=V) for s in _early_docids(V)])
    seen, orig = [], beam_ref.BeamHypotheses.is_done

    def spy(self, best, cur_len):
        d = orig(self, best, cur_len)
        seen.append((id(self), cur_len, d))
        return d
    beam_ref.BeamHypotheses.is_done = spy
    try:
        beam_ref.generate(sd, cfg, torch.from_numpy(ids), torch.from_numpy(mask), 16, restricted_head=True, decode_tree=tree)
    finally:
        beam_ref.BeamHypotheses.is_done = orig
    queries = list(dict.fromkeys(h for h, _c, _d in seen))
    first = {h: min(c for hh, c, d in seen if hh == h and d) for h in queries if any(d for hh, _c, d in seen if hh == h)}
    assert len(queries) == 5 and len(first) == 1 and list(first.values()) == [4], first
