"""Corpus search over live rows on the MI355X: gdr_sim_topk / gdr_sim_topk_bf16 with GDR_SIM_LIVE_MASK in every
form sim_topk_impl has, against two oracles —
  (a) the numpy restatement (tests/live_ref.py): values within oracle/parity_rules.py's tolerance, ids exact wherever adjacent
      reference scores are more than twice the tolerance apart;
  (b) compaction: the UNFLAGGED call of the same B, d, dtype and flags over D[live], ids mapped back through the monotone row map:
      identical ids (ties included) and bit-identical values — a score is a row-local fma chain, it does not depend on the tile a
      row sits in or on its neighbours.  ONE form is held to the parity rule instead (SPLIT_SAMPLE below): the fp32 stream
      kernels, whose sample pass adds a row's dot product in another order than their filter pass —
then the case the sample cannot serve (fewer than k live sample rows), fewer than k live rows in all, the memory contract of the
mode (tests/abi_guard.py), determinism, GDRRetriever.search through the document lifecycle, and graph capture."""
import types

import numpy as np
import pytest
import torch

import expand_ref
import lifecycle_ref
import live_ref
import sim_widths
from abi_guard import guarded, guarded_input, poisoned_workspace
from conftest import order_insensitive_topk_match
from gdr_amd import _ffi, codec, ops, synth
from gdr_amd._ffi import lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu

TOL = 1e-4                         # oracle/parity_rules.py: |got - ref| <= 1e-4 + 1e-4 |ref|, ids exact beyond twice that
LIVE, EXH, NOSTREAM = _ffi.SIM_LIVE_MASK, _ffi.SIM_EXHAUSTIVE, _ffi.SIM_NO_STREAM

# form -> (B, N, d, k, flags, bf16).  d = 64: the tiled GEMM core at every B (the stream kernels need d % 128 == 0, bf16 d % 256 == 0)
FORMS = {
    "stride1_B4": (4, 1000, 64, 10, 0, False),
    "stride1_B40": (40, 1000, 64, 10, 0, False),
    "sampled_B4": (4, 20_000, 64, 10, 0, False),
    "sampled_B40": (40, 20_000, 64, 10, 0, False),
    "stream_sliced_B4": (4, 20_000, 128, 10, 0, False),             # latency mode: stream kernels, sliced threshold / select tails
    "no_stream_B4": (4, 20_000, 128, 10, NOSTREAM, False),          # the same shape forced onto the tiled core
    "ragged_B4": (4, 20_011, 64, 10, 0, False),
    "deep_select_B4": (4, 20_000, 64, 1100, 0, False),              # k > 1024: the deep form of launch_select
    "bf16_B40": (40, 20_000, 64, 10, 0, True),
    "bf16_stream_B4": (4, 20_000, 256, 10, 0, True),
    "exhaustive_B4": (4, 20_000, 64, 10, EXH, False),
}
# The fp32 stream kernels (B <= 32, d % 128 == 0) run a SMALL sample pass — at most 128 x 8 32-row slices, here 20 — as
# sim_stream_sample_splitk_kernel: the waves of a workgroup split d between them and their partial sums are added afterwards, while
# the filter pass (sim_stream_f32_kernel<2>) adds one chain over d.  The bits of a row's score therefore depend on whether its
# tile is a sample tile — in the unflagged call too —, and compaction moves rows between the two kinds of tile.  For this form
# oracle (b) is the parity rule against the compacted call, not bit equality; with nothing dead no row moves and bit equality with
# the unflagged call is still asserted.
SPLIT_SAMPLE = {"stream_sliced_B4"}
MASKS = ("none", "topk_union", "inside_sample_tiles", "outside_sample_tiles", "word_boundaries")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.set_grad_enabled(False)
    return torch.device("cuda:0")


_DATA = {}


def _data(form, dev):
    """Per form, made once and never modified: the operands on host and device, the fp64 scores of the operands as the kernel sees
    them, and the unflagged result.  A few rows are exact copies of a query's best rows, so that exact ties sit inside the top-k."""
    if form not in _DATA:
        B, N, d, k, flags, bf16 = FORMS[form]
        D = synth.make_corpus(N, d, seed=N + d)
        Q, _ = synth.make_queries(D, B, seed=B + d)
        for q in range(min(B, 2)):
            src = np.argsort(-(D @ Q[q]))[:2]
            D[(src + 777) % N] = D[src]
        Qt, Dt = torch.from_numpy(Q), torch.from_numpy(D)
        if bf16:
            Qt, Dt = Qt.bfloat16(), Dt.bfloat16()
        S = live_ref.scores(Qt.double().numpy(), Dt.double().numpy())
        Qd, Dd = Qt.to(dev), Dt.to(dev)
        v0, i0, st0 = _raw(Qd, Dd, k, flags)
        assert int(st0.abs().sum()) == 0
        _DATA[form] = types.SimpleNamespace(form=form, B=B, N=N, d=d, k=k, flags=flags, bf16=bf16, S=S, Qd=Qd, Dd=Dd, v0=v0, i0=i0,
                                            stride=sim_widths.plan(N, k, bool(flags & EXH))[0])
    return _DATA[form]


def _raw(Qd, Dd, k, flags, live=None, idx_offset=0):
    """The C entry point with a workspace of exactly the declared size; live: bool numpy [N] -> the flagged call."""
    B, d = Qd.shape
    N = Dd.shape[0]
    if live is not None:
        flags |= LIVE
    need = lib().gdr_sim_topk_workspace_bytes(B, N, d, k, flags)
    ws = torch.empty(need, dtype=torch.uint8, device=Qd.device)
    if live is not None:
        words = torch.from_numpy(live_ref.pack(live)).to(Qd.device)
        ws[:words.numel() * 4].view(torch.int32).copy_(words)
    v = torch.empty((B, k), dtype=torch.float32, device=Qd.device)
    i = torch.empty((B, k), dtype=torch.int32, device=Qd.device)
    st = torch.empty((B,), dtype=torch.int32, device=Qd.device)
    fn = lib().gdr_sim_topk_bf16 if Qd.dtype == torch.bfloat16 else lib().gdr_sim_topk
    rc = fn(ptr(Qd), B, ptr(Dd), N, d, k, idx_offset, ptr(v), ptr(i), ptr(st), flags, ptr(ws), need, stream_ptr())
    assert rc == 0, lib().gdr_last_error().decode()
    return v, i, st


def _compacted(s, live, k=None):
    """Oracle (b): the unflagged call over D[live], ids mapped back to rows of D."""
    rows = np.nonzero(live)[0]
    cv, ci, cst = _raw(s.Qd, s.Dd[torch.from_numpy(rows).to(s.Dd.device)].contiguous(), k or s.k, s.flags)
    assert int(cst.abs().sum()) == 0
    return cv, rows[ci.cpu().numpy().astype(np.int64)]


def _check(s, live, v, i, what):
    """Both oracles for one flagged result (device tensors v, i without idx_offset)."""
    iv = i.cpu().numpy().astype(np.int64)
    assert live[iv].all(), f"{what}: a dead row was returned"
    rv, ri = live_ref.topk(s.S, live, s.k)
    order_insensitive_topk_match(rv, ri, v.cpu().numpy(), iv, TOL)
    cv, ci = _compacted(s, live)
    if s.form in SPLIT_SAMPLE:
        order_insensitive_topk_match(cv.cpu().numpy(), ci, v.cpu().numpy(), iv, TOL)
        return
    assert np.array_equal(iv, ci), f"{what}: ids differ from the unflagged call over the live rows"
    assert torch.equal(v, cv), f"{what}: values are not the bits of the unflagged call over the live rows"


def _mask(s, name):
    rng = np.random.default_rng(len(name) + s.N)
    live = np.ones(s.N, bool)
    inside = sim_widths.in_sample_tile(s.N, s.stride)
    top = np.unique(s.i0.cpu().numpy())
    if name == "topk_union":
        live[top] = False
    elif name == "inside_sample_tiles":
        live[inside & (rng.random(s.N) < 0.5)] = False
        live[top[inside[top]]] = False
    elif name == "outside_sample_tiles":
        live[~inside & (rng.random(s.N) < 0.3)] = False
        live[top[~inside[top]]] = False
    elif name == "word_boundaries":
        live[:32] = False
        live[-33:] = False
    return live


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("form", list(FORMS))
def test_masked_topk_in_every_form(dev, form, mask):
    s = _data(form, dev)
    assert s.stride == {"stride1_B4": 1, "stride1_B40": 1, "exhaustive_B4": 1, "deep_select_B4": 4}.get(form, 39)
    live = _mask(s, mask)
    assert int(live.sum()) >= s.k
    v, i, st = _raw(s.Qd, s.Dd, s.k, s.flags, live)
    assert int(st.abs().sum()) == 0
    if mask == "none":
        assert torch.equal(v, s.v0) and torch.equal(i, s.i0), "nothing dead: not the unflagged result bit for bit"
    if mask == "topk_union":
        # fails without the feature (bit 4 of flags was ignored): every row of the unfiltered answer is dead
        assert not np.isin(i.cpu().numpy(), s.i0.cpu().numpy()).any()
    _check(s, live, v, i, f"{form} / {mask}")
    # ids are row + idx_offset
    v2, i2, _ = _raw(s.Qd, s.Dd, s.k, s.flags, live, idx_offset=1000)
    assert torch.equal(v2, v) and torch.equal(i2, i + 1000)


@pytest.mark.parametrize("form", ["sampled_B4", "sampled_B40", "stream_sliced_B4", "bf16_B40"])
def test_fewer_than_k_live_sample_rows(dev, form):
    """Every row of every sample tile dead except 5 (k = 10), all other rows live: the k-th largest live sample score does not
    exist, and the smallest of the five is no lower bound of anything.  The raw call then RAISES STATUS for every query
    (sim_live_thr_fixup_kernel lowers thr to -inf, the filter pass keeps all 19 360 other rows and overflows the 6 016-entry list);
    a raw list with status 0 must be the restatement's.  ops.sim_topk re-runs the flagged queries with
    SIM_EXHAUSTIVE | SIM_LIVE_MASK and is exact."""
    s = _data(form, dev)
    assert s.stride == 39 and s.k == 10
    inside = sim_widths.in_sample_tile(s.N, s.stride)
    live = ~inside
    best_inside = np.argsort(-np.where(inside, s.S[0], -np.inf))[:5]          # the five are query 0's best sample rows
    live[best_inside] = True
    assert int((live & inside).sum()) == 5
    rv, ri = live_ref.topk(s.S, live, s.k)
    v, i, st = _raw(s.Qd, s.Dd, s.k, s.flags, live)
    st = st.cpu().numpy()
    assert (st == 1).all(), "the sample gave no threshold: every query must be flagged"
    ok = st == 0                                                              # (none here; the rule for a list that is not flagged)
    order_insensitive_topk_match(rv[ok], ri[ok], v.cpu().numpy()[ok], i.cpu().numpy().astype(np.int64)[ok], TOL)
    L = ops.LiveRows.from_bool(torch.from_numpy(live).to(dev))
    ov, oi, ost = ops.sim_topk(s.Qd, s.Dd, s.k, flags=s.flags, live=L, return_status=True)
    assert int(ost.abs().sum()) == 0
    _check(s, live, ov, oi, f"{form}: ops.sim_topk")
    # exactly k live sample rows: the sample gives a threshold again (a low one — a list may still overflow, and says so)
    live[np.argsort(-np.where(inside, s.S[0], -np.inf))[5:10]] = True
    rv, ri = live_ref.topk(s.S, live, s.k)
    v, i, st = _raw(s.Qd, s.Dd, s.k, s.flags, live)
    ok = st.cpu().numpy() == 0
    order_insensitive_topk_match(rv[ok], ri[ok], v.cpu().numpy()[ok], i.cpu().numpy().astype(np.int64)[ok], TOL)
    L = ops.LiveRows.from_bool(torch.from_numpy(live).to(dev))
    ov, oi = ops.sim_topk(s.Qd, s.Dd, s.k, flags=s.flags, live=L)
    _check(s, live, ov, oi, f"{form}: k live sample rows")


def test_fewer_than_k_live_rows(dev):
    s = _data("stride1_B4", dev)
    live = np.zeros(s.N, bool)
    live[[0, 31, 32, 500, 777, 998, 999]] = True
    rv, ri = live_ref.topk(s.S, live, s.k)
    for form in ("stride1_B4", "stride1_B40"):
        s = _data(form, dev)
        rv, ri = live_ref.topk(s.S, live, s.k)
        v, i, st = _raw(s.Qd, s.Dd, s.k, s.flags, live)
        assert int(st.abs().sum()) == 0
        iv, vv = i.cpu().numpy().astype(np.int64), v.cpu().numpy()
        assert (iv[:, 7:] == -1).all() and np.isneginf(vv[:, 7:]).all(), "the tail of a short list is -inf / -1"
        order_insensitive_topk_match(rv[:, :7], ri[:, :7], vv[:, :7], iv[:, :7], TOL)
        cv, ci = _compacted(s, live, k=7)
        assert np.array_equal(iv[:, :7], ci) and torch.equal(v[:, :7], cv)
        L = ops.LiveRows.from_bool(torch.from_numpy(live).to(dev))
        with pytest.raises(RuntimeError, match="selected index k out of range"):
            ops.sim_topk(s.Qd, s.Dd, s.k, live=L)
        ov, oi = ops.sim_topk(s.Qd, s.Dd, 7, live=L)
        assert torch.equal(ov, v[:, :7]) and torch.equal(oi, i[:, :7])
    with pytest.raises(_ffi.GdrError, match="LiveRows over the 1000 rows"):
        ops.sim_topk(s.Qd, s.Dd, 5, live=ops.LiveRows(999, dev))


def test_prefiltered_corpus_with_live_takes_the_plain_path(dev):
    s = _data("sampled_B40", dev)
    live = _mask(s, "topk_union")
    L = ops.LiveRows.from_bool(torch.from_numpy(live).to(dev))
    P = ops.PrefilteredCorpus(s.Dd)
    pv, pi = ops.sim_topk(s.Qd, P, s.k, live=L)
    ov, oi = ops.sim_topk(s.Qd, s.Dd, s.k, live=L)
    assert torch.equal(pv, ov) and torch.equal(pi, oi)
    _check(s, live, pv, pi, "PrefilteredCorpus + live")


@pytest.mark.parametrize("form", ["ragged_B4", "sampled_B40", "stream_sliced_B4", "stride1_B4"])
def test_memory_contract_of_the_mode(dev, form):
    """A workspace of exactly gdr_sim_topk_workspace_bytes(.., flags | LIVE_MASK) between guard bands: the scratch behind the bitmap
    poisoned, the bitmap region (garbage in the ignored bits past N and in the padding up to 256 bytes) bit-identical after the
    call, guarded outputs, operands with winning rows behind them, a non-default stream."""
    s = _data(form, dev)
    live = _mask(s, "topk_union")
    live[np.random.default_rng(5).random(s.N) < 0.1] = False
    M = (4 * ((s.N + 31) // 32) + 255) // 256 * 256
    flags = s.flags | LIVE
    need = lib().gdr_sim_topk_workspace_bytes(s.B, s.N, s.d, s.k, flags)
    region = torch.full((M,), 0xA7, dtype=torch.uint8)
    words = live_ref.pack(live).copy()
    if s.N % 32:
        words[-1] |= np.int32(-1) << np.int32(s.N % 32)                      # bits past N: ignored
    region[:words.size * 4] = torch.from_numpy(words.view(np.uint8))
    region = region.to(dev)
    far = torch.full((256, s.d), 10.0, dtype=s.Dd.dtype)                      # rows that would win every top-k if read
    Qd, qh = guarded_input(s.Qd.cpu(), tail=torch.full((128, s.d), 1e3, dtype=s.Qd.dtype))
    Dd, dh = guarded_input(s.Dd.cpu(), tail=far)
    fn = lib().gdr_sim_topk_bf16 if s.bf16 else lib().gdr_sim_topk
    side = torch.cuda.Stream(device=dev)
    runs = []
    for fill in (0x00, 0xFF, 0x5A):
        ws, hws = poisoned_workspace(need, fill, dev)
        ws[:M].copy_(region)
        v, hv = guarded((s.B, s.k), torch.float32, dev)
        i, hi = guarded((s.B, s.k), torch.int32, dev)
        st, hst = guarded((s.B,), torch.int32, dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        for rep in range(2 if fill == 0x5A else 1):                           # the last fill runs twice on the warm workspace
            with torch.cuda.stream(side):
                assert stream_ptr().value == side.cuda_stream and side.cuda_stream != 0
                rc = fn(ptr(Qd), s.B, ptr(Dd), s.N, s.d, s.k, 0, ptr(v), ptr(i), ptr(st), flags, ptr(ws), need, stream_ptr())
            assert rc == 0, lib().gdr_last_error().decode()
            side.synchronize()
            tag = f"{form} fill 0x{fill:02X} run {rep}"
            for h, name in ((hws, "workspace"), (hv, "out_val"), (hi, "out_idx"), (hst, "status")):
                h.check(f"{tag}: {name}")
            assert torch.equal(ws[:M], region), f"{tag}: the bitmap region was written"
            runs.append((v.clone(), i.clone(), st.clone()))
    qh.unchanged("Q")
    dh.unchanged("D")
    assert lib().gdr_device_fault_pending() == 0
    for v, i, st in runs:
        assert int(st.abs().sum()) == 0
        assert torch.equal(v, runs[0][0]) and torch.equal(i, runs[0][1]), "the result depends on what the scratch held"
    _check(s, live, runs[0][0], runs[0][1], form)


@pytest.mark.parametrize("form", ["sampled_B40", "stream_sliced_B4", "deep_select_B4"])
def test_two_runs_are_bit_identical(dev, form):
    s = _data(form, dev)
    live = _mask(s, "outside_sample_tiles")
    a, b = _raw(s.Qd, s.Dd, s.k, s.flags, live), _raw(s.Qd, s.Dd, s.k, s.flags, live)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("form", ["sampled_B40", "stream_sliced_B4"])
def test_masked_call_in_a_captured_graph(dev, form):
    """One masked call captured in a graph — the copy of the bitmap into the workspace, the passes, the three mask launches —
    replayed twice; between the replays the LiveRows changes in place, and the replay follows it."""
    s = _data(form, dev)
    live = _mask(s, "topk_union")
    L = ops.LiveRows.from_bool(torch.from_numpy(live).to(dev))
    need = lib().gdr_sim_topk_workspace_bytes(s.B, s.N, s.d, s.k, s.flags | LIVE)
    ws = live_ref.FixedWorkspace(torch.empty(need, dtype=torch.uint8, device=dev))
    call = lambda: ops.sim_topk(s.Qd, s.Dd, s.k, workspace=ws, flags=s.flags, live=L, exact_on_overflow=False, return_status=True)   # noqa: E731
    warm = torch.cuda.Stream(device=dev)
    warm.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(warm):
        ev, ei, est = call()                                                  # eager; also the one run a capture needs first
    torch.cuda.current_stream().wait_stream(warm)
    torch.cuda.synchronize()
    ev, ei = ev.clone(), ei.clone()
    assert int(est.abs().sum()) == 0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gv, gi, gst = call()
    for _ in range(2):
        gv.zero_(), gi.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(gv, ev) and torch.equal(gi, ei) and int(gst.abs().sum()) == 0
    _check(s, live, gv, gi, f"{form}: graph replay")
    more = np.unique(ei.cpu().numpy())                                        # the rows just returned die
    L.clear(more)
    live[more] = False
    g.replay()
    torch.cuda.synchronize()
    assert not np.isin(gi.cpu().numpy(), more).any()
    _check(s, live, gv, gi, f"{form}: graph replay after the mask changed")


# ------------------------------------------------------------------------------------------------ the retriever
def _args(V, R=4):
    return types.SimpleNamespace(num_return_sequences=R, output_vocab_size=V, max_output_length=4, length_penalty=0.8, kary=V,
                                 position=1, score_rate=[0, 1.0], loss_func="tanh")


def test_retriever_search_follows_the_document_lifecycle(dev):
    """remove_documents -> update_documents of some removed ids -> add_documents: after each step GDRRetriever.search is bit-identical
    to DenseModel.search with a LiveRows built fresh from the restated index (tests/lifecycle_ref.py), and no withdrawn id appears."""
    from gdr_amd.modeling import DenseModel, GDRRetriever
    V, csz, d, k, B = 30, 3, 64, 20, 6
    names = ["-".join(str(x) for x in synth.cluster_digits(c, 2, V)) for c in range(V * V)]
    N0 = len(names) * csz
    D0 = synth.make_corpus(N0, d, cluster_size=csz, seed=8)
    Q, _ = synth.make_queries(D0, B, seed=3)
    Qd = torch.from_numpy(Q).to(dev)
    idx = codec.ClusterIndex(names, (np.arange(len(names) + 1) * csz).astype(np.int32), np.arange(N0, dtype=np.int32))
    r = GDRRetriever(None, torch.from_numpy(D0).to(dev), idx, _args(V))
    dense = DenseModel(None)

    def fresh(offs, mem):
        N = r.doc_embed.shape[0]
        live = np.zeros(N, bool)
        live[np.asarray(mem)] = True
        assert np.array_equal(r.index.offsets, offs) and np.array_equal(r.index.members, mem)
        L = ops.LiveRows.from_bool(torch.from_numpy(live).to(dev))
        assert torch.equal(r.live_rows.words, L.words) and r.live_rows.count == L.count == int(live.sum()) and r.live_rows.n == N
        v, i = r.search(Qd, k)
        fv, fi = dense.search(Qd, r.doc_embed, k, live=L)
        assert i.dtype == torch.int64 and torch.equal(v, fv) and torch.equal(i, fi)
        rv, ri = live_ref.topk(live_ref.scores(Q, r.doc_embed.cpu().numpy()), live, k)
        order_insensitive_topk_match(rv, ri, v.cpu().numpy(), i.cpu().numpy(), TOL)
        return i.cpu().numpy()

    offs, mem = idx.offsets, idx.members
    base = fresh(offs, mem)                                                   # live_rows is built here, from the index as built
    uv, ui = ops.sim_topk(Qd, r.doc_embed, k)
    assert np.array_equal(base, ui.cpu().numpy())                             # nothing withdrawn yet: the plain search
    gone = np.unique(np.concatenate([base[:, :5].reshape(-1), np.arange(0, N0, 7), np.arange(N0 - 40, N0)]))
    offs, mem, n = lifecycle_ref.remove(offs, mem, gone)
    assert r.remove_documents(gone) == n
    got = fresh(offs, mem)
    assert not np.isin(got, gone).any(), "a removed document came back from the corpus search"
    back = gone[::3]
    cl = r.update_documents(back, torch.from_numpy(D0[back]).to(dev))         # restored, with their old embeddings
    offs, mem = lifecycle_ref.update(offs, mem, back, cl)
    got = fresh(offs, mem)
    still = np.setdiff1d(gone, back)
    assert not np.isin(got, still).any() and np.isin(got, back).any()
    X = (D0[base[:, 0]] * np.float32(1.01)).astype(np.float32)                # every query's old best document again, a little longer
    new_ids, cl = r.add_documents(torch.from_numpy(X).to(dev))
    offs, mem = expand_ref.merge(offs, mem, new_ids, cl)
    got = fresh(offs, mem)
    assert r.doc_embed.shape[0] == N0 + B and np.isin(got, new_ids).any() and not np.isin(got, still).any()
    sh = GDRRetriever(None, r.doc_embed, r.index, _args(V), sharded=types.SimpleNamespace(D=r.doc_embed))
    with pytest.raises(_ffi.GdrError, match="sharded"):
        sh.search(Qd, k)
