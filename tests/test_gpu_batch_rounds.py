"""Batches past one round of the one-workgroup plan kernels (cases, builders and references: tests/batch_rounds.py; their premises on the
CPU: tests/test_batch_rounds_host.py).  The scans are csrc/scan.h's: the round form (BlockScan<1024>::round per 1024 entries, a carry
between the rounds; rows_units_kernel is that loop written out) and the single-shot form (block_scan_once over the 1024 thread sums of
ceil(n / 1024) consecutive entries each).  Which case enters which round count:

pack_scan_kernel (csrc/layers.hip; round form) — every packed forward of both towers:
  B = 1023, L = 24    one partial round (threads 1023 idle)
  B = 1024, L = 24    exactly one round
  B = 1025, L = 24    two rounds, the second with one sequence; pooled-only fp32 T5 stays one chain (the halves do not pack)
  B = 2049, L = 24    three rounds; the pooled-only fp32 T5 call splits into chains of 1024 (one round) and 1025 (two rounds)
  B = 1025, L = 130   two rounds; the key-block attention of attention_long.hip reads seq_off past round one (fp32 forms)
  forms: T5 fp32 / bf16 and the doc tower's fp32 bit for bit against the padded form of the same handle (which has no plan);
  T5 split 6 / 3 / 2 terms and the doc tower's bf16 / split against the float64 CPU oracle on the sequences on either side of
  every round boundary, the split forms also against the fp32 packed form on every sequence.
rows_units_kernel (csrc/sim_rows.hip; round form) — ops.sim_topk(gather=4096), fp32 and bf16 corpus:
  B = 1024            exactly one round
  B = 1025            two rounds, the second with one query
  B = 2050            three rounds, the third with two queries
  every query against the same call on slices of <= 512 queries (one round each), the sampled ones against float64 scores.
prefix_plan_kernel (csrc/decode.hip; single-shot form, per = ceil(rows / 1024) consecutive rows per thread) — generate() with a prefix table:
  B = 171, R = 6      1026 rows: per = 2, threads 0 .. 512 own rows
  B = 350, R = 6      2100 rows: per = 3, threads 0 .. 699 own rows
  both with holes in the trie's second level (keep_every 3 and 7): hit and miss rows inside one thread's rows at step 2.
insert_scan_kernel (csrc/cluster_insert.hip; single-shot form over int64 sums, per = ceil(C / 1024) clusters per thread, a block maximum
  beside it) — test_gpu_expand.py reaches C = 2000 through add_documents, but only compares one call with three; test_gpu_lifecycle.py
  removes from 9 clusters.  Two cases at C = 2049 (per = 3, threads 0 .. 682 own clusters):
  insert          against expand_ref.merge exactly.
  removal         a negative histogram, clusters emptied on either side of the thread boundaries, an id in no cluster: against
                  lifecycle_ref.remove exactly, out_max = the largest surviving cluster.
part_scan_kernel (csrc/kmeans.hip; single-shot form) at 1024 / 1025 / 1023 scan entries: tests/test_gpu_kmeans.py
  test_partition_is_a_stable_counting_sort (batch_rounds.PARTITION_CASES).  cluster_candidates_kernel (csrc/rerank.hip; round form at
  256 threads) at R = 256 / 257: tests/test_gpu_rerank.py test_cluster_candidates_on_either_side_of_one_scan_round.
"""
import gc

import numpy as np
import pytest
import torch

import batch_rounds as BR
import expand_ref
import peaked
from gdr_amd._ffi import lib
from oracle.parity_rules import beam_cut_explains_absence, hypothesis_lists_match, order_insensitive_topk_match

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _no_fault():
    torch.cuda.synchronize()
    assert lib().gdr_device_fault_pending() == 0


# ==================================================================================================== 1. pack plan
_HANDLES = {}


@pytest.fixture(scope="module", autouse=True)
def _handles_live_for_this_module_only(dev):
    """The handles keep their workspaces (several GB at 1025 x 130): dropped with the module, so that later modules — the ones that
    fill most of the device's memory among them — start from what they started from before."""
    gc.collect()
    before = torch.cuda.memory_allocated()
    yield
    _HANDLES.clear()
    gc.collect()
    torch.cuda.synchronize()
    left = torch.cuda.memory_allocated() - before
    print(f"test_gpu_batch_rounds: {left} bytes more allocated after the module than before it")
    assert left < 64 << 20, f"the module leaves {left} bytes allocated on the device"


def _handle(form, dev):
    """One handle per form for the module: the weights go to the device once."""
    from gdr_amd import ops
    if form not in _HANDLES:
        row = BR.TOWER_FORMS[form]
        if row["tower"] == "t5":
            _HANDLES[form] = ops.T5EncoderHandle(BR.t5_config(), BR.t5_state_dict(), dev, **row["kw"])
        else:
            _HANDLES[form] = ops.BertEncoderHandle(BR.bert_cfg(), BR.bert_state_dict(), dev, **row["kw"])
    return _HANDLES[form]


def _tokens(form, B, L, dev):
    vocab = BR.t5_config().vocab_size if BR.TOWER_FORMS[form]["tower"] == "t5" else BR.bert_cfg()["vocab_size"]
    ids, mask = BR.tower_tokens(B, L, vocab)
    return mask, torch.from_numpy(np.array(ids)).to(dev), torch.from_numpy(np.array(mask)).to(dev)


def _twice(call):
    """The call, the fault flag, the call again: the second run reproduces the first bit for bit."""
    h1, p1 = call()
    _no_fault()
    h2, p2 = call()
    _no_fault()
    for a, b in ((h1, h2), (p1, p2)):
        assert (a is None and b is None) or torch.equal(a, b), "two runs of one call differ"
    return h1, p1


# the L = 130 case is set for the fp32 forms
_T5_EXACT = [(form, B, L) for form in ("t5-fp32", "t5-bf16") for B, L in BR.tower_shapes() if form == "t5-fp32" or (B, L) != BR.TOWER_LONG]


@pytest.mark.parametrize("form,B,L", _T5_EXACT)
def test_t5_packed_form_is_the_padded_form_bit_for_bit(dev, form, B, L):
    """With hidden output, pooled-only and want_pooled=False: every kept row and every pooled row equals the padded form of the same
    handle, dropped rows are zero.  The padded form has no pack plan."""
    assert BR.t5_packs(BR.t5_config(), B, L) and BR.rounds(B) == (B + 1023) // 1024
    enc = _handle(form, dev)
    mask, it, mt = _tokens(form, B, L, dev)
    h0, p0 = enc.forward(it, mt)
    _no_fault()
    h1, p1 = _twice(lambda: enc.forward(it, mt, ragged=True, live_rows_hint=int(BR.kept(mask).sum())))
    hn, p2 = _twice(lambda: enc.forward(it, mt, ragged=True, want_hidden=False))
    h3, pn = _twice(lambda: enc.forward(it, mt, ragged=True, want_pooled=False))
    assert hn is None and pn is None
    keep = torch.from_numpy(BR.kept(mask)).to(dev)
    assert torch.equal(p1, p0), "pooled (hidden + pooled call)"
    assert torch.equal(p2, p0), f"pooled (pooled-only call: chains of {BR.t5_chains(BR.t5_config(), B, L)} sequences)"
    assert torch.equal(h1[keep], h0[keep]), "kept hidden rows"
    assert int((h1[~keep] != 0).sum()) == 0, "dropped rows are zero"
    assert torch.equal(h3, h1)
    assert float(h0[~keep].abs().max()) > 0                   # the padded form did compute the dropped rows


@pytest.mark.parametrize("B,L", BR.tower_shapes())
def test_doc_tower_packed_form_is_the_padded_form_bit_for_bit(dev, B, L):
    assert BR.bert_packs(BR.bert_cfg(), B, L)
    enc = _handle("bert-fp32", dev)
    mask, it, mt = _tokens("bert-fp32", B, L, dev)
    h0, p0 = enc.forward(it, mt, ragged=False)
    _no_fault()
    h1, p1 = _twice(lambda: enc.forward(it, mt, ragged=True, live_rows_hint=int(BR.kept(mask).sum())))
    hn, p2 = _twice(lambda: enc.forward(it, mt, ragged=True, want_hidden=False))
    assert hn is None
    keep = torch.from_numpy(BR.kept(mask)).to(dev)
    assert torch.equal(p1, p0) and torch.equal(p2, p0), "pooled output of the packed form differs from the padded form"
    assert torch.equal(h1[keep], h0[keep]), "kept hidden rows"
    assert int((h1[~keep] != 0).sum()) == 0, "dropped rows are zero"
    assert float(h0[~keep].abs().max()) > 0


def _close(got, want, bound, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    print(f"{what}: max |gpu - oracle| {np.abs(got - want).max():.2e} (bound {bound:.1e})")
    np.testing.assert_allclose(got, want, rtol=bound, atol=bound, err_msg=what)


@pytest.mark.parametrize("B", BR.TOWER_BATCHES)
@pytest.mark.parametrize("form", ["t5-split6", "t5-split3", "t5-split2", "bert-split", "bert-bf16"])
def test_packed_only_forms_against_the_float64_oracle(dev, form, B):
    """The forms without a padded counterpart.  Sample: the sequences on either side of every round boundary, the first and the last
    — a wrong carry moves every sequence behind it onto other sequences' rows.  Split forms: oracle/t5_ref.py, oracle/bert_ref.py in
    float64 at the bound of the form's existing test, and the pooled rows of EVERY sequence within that test's cap of the fp32 packed
    form's (which the tests above hold to the padded form).  bert-bf16: the oracle's bf16 emulation with float64 sums, 4 x the
    recorded distance between that emulation with fp32 and with float64 sums (batch_rounds.BERT_BF16_NOISE)."""
    row, L = BR.TOWER_FORMS[form], BR.TOWER_L
    tower, bf16 = row["tower"], row.get("bf16", False)
    enc = _handle(form, dev)
    mask, it, mt = _tokens(form, B, L, dev)
    h1, p1 = _twice(lambda: enc.forward(it, mt, ragged=True, live_rows_hint=int(BR.kept(mask).sum())))
    _, p2 = _twice(lambda: enc.forward(it, mt, ragged=True, want_hidden=False))
    keep_all = torch.from_numpy(BR.kept(mask)).to(dev)
    assert int((h1[~keep_all] != 0).sum()) == 0, "dropped rows are zero"
    assert bool(torch.isfinite(h1).all()) and bool(torch.isfinite(p2).all())
    rows, _, _, keep, ref = BR.tower_sample(tower, B, L, bf16, True)
    got_h, got_p, got_p2 = h1[rows].cpu().numpy(), p1[rows].cpu().numpy(), p2[rows].cpu().numpy()
    what = f"{form} B={B} sequences {rows}"
    if bf16:
        mx, mean = (row["margin"] * x for x in row["measured"])
        d = np.abs(got_h.astype(np.float64) - ref)[keep]
        dp = max(np.abs(got_p - ref[:, 0]).max(), np.abs(got_p2 - ref[:, 0]).max())
        print(f"{what}: |gpu - bf16 emulation with float64 sums| max {d.max():.3e} mean {d.mean():.3e} pooled {dp:.3e} "
              f"(bounds {mx:.1e} / {mean:.1e})")
        assert d.max() <= mx and d.mean() <= mean and dp <= mx, what
    else:
        _close(got_h[keep], ref[keep], row["bound"], what + " hidden (kept rows)")
        _close(got_p, ref[:, 0], row["bound"], what + " pooled")
        _close(got_p2, ref[:, 0], row["bound"], what + " pooled-only")
    assert float((p2 - p1).abs().max()) <= 1e-5               # the CLS tail gives the same numbers (test_gpu_decode.py, both forms)
    if "vs_fp32" in row:
        fp32 = _handle(f"{tower}-fp32", dev)
        h32, p32 = fp32.forward(it, mt, ragged=True)
        dp, dh = float((p1 - p32).abs().max()), float((h1 - h32).abs().max())
        print(f"{form} B={B}: every sequence against the fp32 packed form: max |pooled| {dp:.2e} (cap {row['vs_fp32']:.0e}), "
              f"|hidden| {dh:.2e} (cap 2e-4)")
        assert dp <= row["vs_fp32"] and float((p2 - p32).abs().max()) <= row["vs_fp32"] and dh <= 2e-4


# ==================================================================================================== 2. gather top-k
def _gather_call(Qd, Dd, R, **kw):
    from gdr_amd import ops
    return ops.sim_topk(Qd, Dd, BR.GATHER_K, allowed=R, gather=BR.GATHER_CAP, exact_on_overflow=False, return_status=True, **kw)


@pytest.mark.parametrize("B", BR.GATHER_BATCHES)
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_gather_topk_past_one_round_of_queries(dev, bf16, B):
    from gdr_amd import ops
    s = BR.gather_case(B, bf16)
    a, k, cap = s.allowed, s.k, BR.GATHER_CAP
    Qd, Dd = s.Qt.to(dev), s.Dt.to(dev)
    R = ops.QueryRows.from_bool(torch.from_numpy(np.array(a)).to(dev))
    v, i, st = _gather_call(Qd, Dd, R)
    _no_fault()
    again = _gather_call(Qd, Dd, R)
    assert all(torch.equal(x, y) for x, y in zip(again, (v, i, st))), "two runs differ"
    # (a) a score is a function of the two vectors and d alone: every query equals its row of a call that stays inside one round
    for lo in range(0, B, BR.GATHER_SLICE):
        idx = torch.arange(lo, min(B, lo + BR.GATHER_SLICE), device=dev)
        v1, i1, st1 = _gather_call(Qd[idx].contiguous(), Dd, R.rows(idx))
        for name, whole, part in (("values", v, v1), ("ids", i, i1), ("status", st, st1)):
            bad = (whole[idx] != part).reshape(idx.numel(), -1).any(1).nonzero().flatten()
            assert bad.numel() == 0, f"{name} of queries {(bad[:8] + lo).tolist()} differ from the call on queries {lo} .. {lo + idx.numel() - 1}"
    _no_fault()
    vv, iv, stn = v.cpu().numpy(), i.cpu().numpy().astype(np.int64), st.cpu().numpy()
    counts = a.sum(1)
    # (c) status, (d) empty filters
    assert np.array_equal(stn != 0, counts > cap) and set(np.unique(stn).tolist()) <= {0, 1}, "status is 1 exactly where the count exceeds 4096"
    empty = np.nonzero(counts == 0)[0]
    assert empty.tolist() == sorted(q for q, c in BR.gather_designed_counts(B).items() if c == 0)
    assert np.isneginf(vv[empty]).all() and (iv[empty] == -1).all(), "a query with no allowed row returns -inf / -1 in all k slots"
    # (b) the sampled queries against float64 scores over their first 4096 allowed rows
    BR.check_topk_rows(s.S, a, s.sample, vv[s.sample], iv[s.sample], k, cap, f"gather B={B} bf16={bf16}")
    # (e) the dense masked call on the same batch
    dv, di = ops.sim_topk(Qd, Dd, k, allowed=R)
    _no_fault()
    dvv, div = dv.cpu().numpy(), di.cpu().numpy().astype(np.int64)
    BR.check_topk_rows(s.S, a, s.sample, dvv[s.sample], div[s.sample], k, 2 ** 20, f"dense masked B={B} bf16={bf16}")
    for q in np.nonzero(stn == 0)[0]:
        c = int(min(counts[q], k))
        assert (div[q, c:] == -1).all() and np.isneginf(dvv[q, c:]).all()
        order_insensitive_topk_match(vv[q:q + 1, :c], iv[q:q + 1, :c], dvv[q:q + 1, :c], div[q:q + 1, :c], BR.GATHER_TOL)


# ==================================================================================================== 3. prefix-table decode
def _lists_against_oracle(B, dec, sc, what):
    """peaked_gpu.generate_vs_oracle's rule at PREFIX_TOL.  Returns bool [B]: the queries with a hypothesis at another rank or outside
    the oracle's list — each one explained by a gap of the float64 scores below the tolerance, or the rule raises."""
    R, cfg = BR.PREFIX_R, BR.prefix_config()
    ref, ref_sc, trace, ptrace = BR.prefix_oracle(B)
    sc = np.array(sc, np.float64).reshape(B, R)
    np.testing.assert_allclose(sc, ref_sc, rtol=BR.PREFIX_TOL, atol=BR.PREFIX_TOL, err_msg=what)
    got = peaked.hypothesis_lists(dec.cpu().numpy(), B, R)
    excused, moved, foreign = np.zeros(B, bool), 0, 0
    for b in range(B):
        def explain(hyp, b=b):
            return beam_cut_explains_absence(trace, ptrace, b, R, cfg.decode_vocab_size, list(hyp), BR.PREFIX_TOL, final_cut=ref_sc[b, -1])
        m, f, _ = hypothesis_lists_match(ref[b], ref_sc[b], got[b], BR.PREFIX_TOL, explain_foreign=explain)
        excused[b] = m + f > 0
        moved, foreign = moved + m, foreign + f
    print(f"{what}: of {B * R} hypotheses {moved} moved inside a tie group, {foreign} crossed a cut by a tie")
    assert moved + foreign <= BR.PREFIX_MAX_EXCUSED * B * R, what
    return excused, got, sc


@pytest.mark.parametrize("keep_every", BR.PREFIX_KEEP_EVERY)
@pytest.mark.parametrize("B", list(BR.PREFIX_BATCHES))
def test_prefix_table_decode_past_1024_beam_rows(dev, B, keep_every):
    from gdr_amd.modeling import GDRModel
    cfg, sd, R = BR.prefix_config(), BR.prefix_state_dict(), BR.PREFIX_R
    rows, per, _ = BR.PREFIX_BATCHES[B]
    assert B * R == rows > 1024 and per == (rows + 1023) // 1024
    ids, mask = BR.prefix_tokens(B)
    it, mt = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)
    kw = dict(attention_mask=mt, max_length=cfg.max_output_length, num_beams=R, length_penalty=0.8, num_return_sequences=R,
              output_scores=True)
    tabled = GDRModel(cfg, sd, dev, prefix_trie=BR.prefix_trie(keep_every))       # unconstrained: the beams leave the trie and miss
    assert tabled.prefix_table.complete_levels == 2                               # hit and miss rows share the later steps
    (d1, s1), _ = tabled.generate(it, **kw)
    _no_fault()
    (d2, s2), _ = tabled.generate(it, **kw)
    _no_fault()
    assert torch.equal(d1, d2) and s1 == s2, "a second tabled call differs"
    (d0, s0), _ = GDRModel(cfg, sd, dev).generate(it, **kw)
    _no_fault()
    ex1, l1, sc1 = _lists_against_oracle(B, d1, s1, f"prefix table B={B} keep_every={keep_every}")
    ex0, l0, sc0 = _lists_against_oracle(B, d0, s0, f"no table B={B}")
    # against the table-less path: outside the queries whose float64 scores excused a difference above, the same ids, and
    # scores at the tolerance tests/test_gpu_prefix.py holds the two paths to
    same = ~(ex1 | ex0)
    for b in np.nonzero(same)[0]:
        assert l1[b] == l0[b], ("the tabled and the table-less decode differ where the oracle has no near-tie", b, l1[b], l0[b])
    np.testing.assert_allclose(sc1[same], sc0[same], rtol=1e-5, atol=1e-5)


# ==================================================================================================== 4. cluster insert
def test_cluster_insert_at_2049_clusters(dev):
    from gdr_amd import ops
    offsets, members, new_ids, targets = BR.insert_case()
    want_o, want_m = expand_ref.merge(offsets, members, new_ids, targets)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)   # noqa: E731
    for _ in range(2):
        o, m, mx = ops.cluster_insert(up(offsets), up(members), up(new_ids), up(targets))
        _no_fault()
        assert np.array_equal(o.cpu().numpy(), want_o), "offsets differ from tests/expand_ref.py"
        assert np.array_equal(m.cpu().numpy(), want_m), "members differ from tests/expand_ref.py"
        assert mx == int(np.diff(want_o).max())


def test_cluster_remove_at_2049_clusters(dev):
    """insert_scan_kernel over a NEGATIVE histogram (the removal mode) at per = 3: clusters emptied on either side of the thread
    boundaries, an id that is in no cluster; against tests/lifecycle_ref.py exactly, the largest SURVIVING cluster included."""
    import lifecycle_ref
    from gdr_amd import ops
    offsets, members, ids = BR.remove_case()
    want_o, want_m, want_n = lifecycle_ref.remove(offsets, members, ids)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)   # noqa: E731
    for _ in range(2):
        o, m, mx, gone = ops.cluster_remove(up(offsets), up(members), up(ids))
        _no_fault()
        assert np.array_equal(o.cpu().numpy(), want_o), "offsets differ from tests/lifecycle_ref.py"
        assert np.array_equal(m.cpu().numpy(), want_m), "members differ from tests/lifecycle_ref.py"
        assert mx == int(np.diff(want_o).max()) and gone == want_n == ids.size - 1
