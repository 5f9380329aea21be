"""The gather mode of the filtered corpus search on the MI355X: gdr_sim_topk / gdr_sim_topk_bf16 with
GDR_SIM_QUERY_MASK | GDR_SIM_ROW_GATHER, the raw entry point called with a workspace of exactly the declared size, against
  (1) tests/gather_ref.py on fp64 scores of the operands as the kernel sees them (bf16 already rounded), under
      oracle/parity_rules.py's rule with the tolerance tests/test_gpu_live_search.py uses.  No case is skipped.  In the 4-query,
      k = 10 cases the reference's own gap between its k-th and (k + 1)-th score among the ranked rows is asserted to exceed the
      rule's tie width 2 TOL (1 + |score|) for every query and filter, so the id comparison is total there (QSEED: the query seeds
      were chosen on the CPU for that);
  (2) bit for bit: row q of a 40-query call against the one-query call with its bitmap, one sort (c = 2) against chunks plus merge
      rounds (c = 3), two runs, a non-default stream;
  (3) the ids of the GDR_SIM_EXHAUSTIVE | GDR_SIM_QUERY_MASK call, for every query whose reference list has no tolerance-tie group
— then the memory contract (tests/abi_guard.py), graph capture, and the Python surface (ops.sim_topk(gather=), DenseModel.search,
GDRRetriever.search)."""
import types
import zlib

import numpy as np
import pytest
import torch

import gather_ref
import lifecycle_ref
import live_ref
from abi_guard import guarded, guarded_input, poisoned_workspace
from conftest import order_insensitive_topk_match
from gdr_amd import _ffi, codec, ops, synth
from gdr_amd._ffi import lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu

TOL = 1e-4                         # oracle/parity_rules.py: |got - ref| <= 1e-4 + 1e-4 |ref|, ids exact beyond twice that
QM, RG, EXH = _ffi.SIM_QUERY_MASK, 16, _ffi.SIM_EXHAUSTIVE

# form -> (B, N, d, k, bf16).  N = 20 001: the last bitmap word holds one row.  d = 64: fewer 16-byte pieces per row than lanes;
# d = 132: a ragged last sweep of the lanes (33 pieces); bf16 d = 72: 9 pieces.
FORMS = {
    "B4_d64": (4, 20_001, 64, 10, False),
    "B4_d128": (4, 20_001, 128, 10, False),
    "B4_d132": (4, 20_001, 132, 10, False),
    "bf16_B4_d72": (4, 20_001, 72, 10, True),
    "bf16_B4_d256": (4, 20_001, 256, 10, True),
    "B4_N5000_d768": (4, 5000, 768, 10, False),
    "B4_N40000_d64": (4, 40_000, 64, 10, False),                   # more rows than ops.GATHER_MAX_ROWS: an unrestricted query is wide
    "B1_d128": (1, 20_001, 128, 10, False),
    "B40_d128": (40, 20_001, 128, 10, False),
    "bf16_B40_d256": (40, 20_001, 256, 10, True),
    "chunked_B2": (2, 40_000, 64, 10, False),
    "all_rows_B2": (2, 70_001, 64, 1024, False),
}
QSEED = {"B4_d64": 1, "B4_d128": 5}   # form -> query seed, where the default (B + d) leaves a reference tie at a cut (chosen on the CPU)
# a call of a 4-query form: (chunk field, one filter per query)
GROUPS = {
    "edges": (1, ("empty", "one_row", "row_0", "row_last")),
    "k_rows": (1, ("bit_31", "k_minus_1", "k", "k_plus_1")),
    "ties": (2, ("ties", "two_percent", "ties", "k_plus_1")),
    "capacity": (1, ("cap", "cap_plus_1", "two_percent", "empty")),
    "default_field": (0, ("two_percent", "one_row", "cap", "bit_31")),
    "chunks": (3, ("fifty_percent", "two_percent", "k", "cap")),
}
FILTERS = ("empty", "one_row", "row_0", "row_last", "bit_31", "k_minus_1", "k", "k_plus_1", "two_percent", "fifty_percent", "ties",
           "cap", "cap_plus_1")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.set_grad_enabled(False)
    return torch.device("cuda:0")


_HOST, _DATA = {}, {}


def _host(form):
    """Per form, made once and never modified, on the host: the operands and the fp64 scores of the operands as the kernel sees
    them.  The two best rows of queries 0 and 1 have exact copies elsewhere in the corpus (s.dups): exact ties inside a top-k."""
    if form not in _HOST:
        B, N, d, k, bf16 = FORMS[form]
        D = synth.make_corpus(N, d, seed=N + d)
        Q, _ = synth.make_queries(D, B, seed=QSEED.get(form, B + d))
        dups = {}
        for q in range(min(B, 2)):
            src = np.argsort(-(D @ Q[q]))[:2]
            D[(src + 777) % N] = D[src]
            dups[q] = np.concatenate([src, (src + 777) % N])
        Qt, Dt = torch.from_numpy(Q), torch.from_numpy(D)
        if bf16:
            Qt, Dt = Qt.bfloat16(), Dt.bfloat16()
        S = live_ref.scores(Qt.double().numpy(), Dt.double().numpy())
        _HOST[form] = types.SimpleNamespace(form=form, B=B, N=N, d=d, k=k, bf16=bf16, S=S, Qt=Qt, Dt=Dt, dups=dups)
    return _HOST[form]


def _data(form, dev):
    if form not in _DATA:
        s = types.SimpleNamespace(**vars(_host(form)))
        s.Qd, s.Dd = s.Qt.to(dev), s.Dt.to(dev)
        _DATA[form] = s
    return _DATA[form]


def _filter(s, name, q, cap):
    """bool [N]: the rows query q is allowed under the filter `name`; cap: the call's capacity (the cap / cap_plus_1 filters)."""
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 31 * s.N + 7 * s.d + q)
    a = np.zeros(s.N, bool)
    pick = lambda n: rng.choice(s.N, size=n, replace=False)   # noqa: E731
    if name == "empty":
        pass
    elif name == "one_row":
        a[pick(1)] = True
    elif name == "row_0":
        a[0] = True
    elif name == "row_last":
        a[s.N - 1] = True
    elif name == "bit_31":
        a[31::32] = True
    elif name in ("k_minus_1", "k", "k_plus_1"):
        a[pick(s.k + {"k_minus_1": -1, "k": 0, "k_plus_1": 1}[name])] = True
    elif name == "two_percent":
        a[:] = rng.random(s.N) < 0.02
    elif name == "fifty_percent":
        a[:] = rng.random(s.N) < 0.5
    elif name == "ties":
        a[:] = rng.random(s.N) < 0.02
        if q in s.dups:
            a[s.dups[q]] = True
    elif name == "seven_rows":
        a[[0, 31, 32, 4000, 4777, s.N - 2, s.N - 1]] = True
    elif name == "all":
        a[:] = True
    elif name in ("cap", "cap_plus_1"):
        a[pick(min(s.N, cap + (name == "cap_plus_1")))] = True
    else:
        raise KeyError(name)
    return a


def _allowed(s, names, cap):
    return np.stack([_filter(s, names[q % len(names)], q, cap) for q in range(s.B)])


def _flags(c):
    return QM | RG | _ffi.sim_gather_chunks(c)


def _fill_bitmaps(ws, allowed, N):
    B, M, W = allowed.shape[0], live_ref.mask_bytes(N), (N + 31) // 32
    words = torch.from_numpy(np.stack([live_ref.pack(a) for a in allowed])).to(ws.device)
    ws[:B * M].view(torch.int32).view(B, M // 4)[:, :W].copy_(words)


def _raw(Qd, Dd, k, allowed, c=None, idx_offset=0, flags=None, status=True):
    """The C entry point with a workspace of exactly the declared size.  allowed: bool numpy [B, N]; c: the chunk field of a gather
    call, or flags: any other GDR_SIM_QUERY_MASK call."""
    B, d = Qd.shape
    N = Dd.shape[0]
    if flags is None:
        flags = _flags(c)
    need = lib().gdr_sim_topk_workspace_bytes(B, N, d, k, flags)
    if flags & RG:      # fails without the feature (the bits were ignored: the dense plan, which moves with N)
        assert need - B * live_ref.mask_bytes(N) == lib().gdr_sim_topk_workspace_bytes(B, N + 40_960, d, k, flags) - B * live_ref.mask_bytes(N + 40_960) > 0, \
            "the gather layout behind the bitmaps does not depend on N"
    ws = torch.empty(need, dtype=torch.uint8, device=Qd.device)
    _fill_bitmaps(ws, allowed, N)
    v = torch.empty((B, k), dtype=torch.float32, device=Qd.device)
    i = torch.empty((B, k), dtype=torch.int32, device=Qd.device)
    st = torch.full((B,), -7, dtype=torch.int32, device=Qd.device)
    fn = lib().gdr_sim_topk_bf16 if Qd.dtype == torch.bfloat16 else lib().gdr_sim_topk
    rc = fn(ptr(Qd), B, ptr(Dd), N, d, k, idx_offset, ptr(v), ptr(i), ptr(st) if status else None, flags, ptr(ws), need, stream_ptr())
    assert rc == 0, lib().gdr_last_error().decode()
    return v, i, st


def _gap_ok(S, rows, k):
    """The k-th and (k + 1)-th best scores over `rows` are further apart than the parity rule's tie width."""
    v = np.sort(S[rows])[::-1]
    return v.size <= k or bool(v[k - 1] - v[k] > 2 * TOL * (1 + abs(v[k - 1])))


def _check(s, a, cap, v, i, st, what, idx_offset=0, k=None, strict=False):
    """Oracle 1 and the status contract.  Returns bool [B]: the queries whose reference list (its k + 1 best) has no tolerance-tie
    group and whose status is 0 — the ones oracle 3 compares by id."""
    k = k or s.k
    vv, iv, stn = v.cpu().numpy(), i.cpu().numpy().astype(np.int64), st.cpu().numpy()
    rv, ri, rst = gather_ref.topk(s.S, a, k, cap)
    assert stn.tolist() == rst.tolist(), f"{what}: status {stn.tolist()}, expected {rst.tolist()}"
    clean = np.zeros(s.B, bool)
    for q in range(s.B):
        rows, _ = gather_ref.rows_of(live_ref.pack(a[q]), s.N, cap)
        c = int(min(rows.size, k))
        assert (iv[q, c:] == -1).all() and np.isneginf(vv[q, c:]).all(), f"{what}: query {q}: the tail of a short list is -inf / -1"
        got = iv[q, :c] - idx_offset
        assert (got >= 0).all() and (got < s.N).all() and np.isin(got, rows).all(), f"{what}: query {q} was given a row outside its ranked rows"
        if strict:
            assert _gap_ok(s.S[q], rows, k), f"{what}: query {q}: the reference has a tie at the cut; choose another seed"
        order_insensitive_topk_match(rv[q:q + 1, :c], ri[q:q + 1, :c], vv[q:q + 1, :c], got[None], TOL)
        top = np.sort(s.S[q, rows])[::-1][:k + 1]
        clean[q] = stn[q] == 0 and bool((top[:-1] - top[1:] > 2 * TOL * (1 + np.abs(top[:-1]))).all())
    return clean


def _check_against_exhaustive(s, a, i, clean, k=None):
    """Oracle 3."""
    _, ei, est = _raw(s.Qd, s.Dd, k or s.k, a, flags=QM | EXH)
    assert int(est.abs().sum()) == 0
    for q in np.nonzero(clean)[0]:
        assert torch.equal(i[q], ei[q]), f"query {q}: ids differ from the GDR_SIM_EXHAUSTIVE | GDR_SIM_QUERY_MASK call"


@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("form", ["B4_d64", "B4_d128", "B4_d132", "bf16_B4_d72", "bf16_B4_d256"])
def test_four_queries_with_a_filter_each(dev, form, group):
    s = _data(form, dev)
    c, names = GROUPS[group]
    cap = gather_ref.cap_of(c)
    a = _allowed(s, names, cap)
    v, i, st = _raw(s.Qd, s.Dd, s.k, a, c)
    clean = _check(s, a, cap, v, i, st, f"{form} / {group}", strict=True)
    _check_against_exhaustive(s, a, i, clean)
    if group == "ties":                                                       # exact copies inside the top-k: the lower id first
        iv = i.cpu().numpy()
        for q in (0, 2 % s.B):
            if names[q] == "ties" and q in s.dups:
                src, cp = s.dups[q][:2], s.dups[q][2:]
                for x, y in zip(src, cp):
                    px, py = np.nonzero(iv[q] == x)[0], np.nonzero(iv[q] == y)[0]
                    assert px.size == 1 and py.size == 1 and abs(int(px[0]) - int(py[0])) == 1 and (px[0] < py[0]) == (x < y)
                    assert float(v[q, px[0]]) == float(v[q, py[0]])
    if group == "capacity":
        assert st.cpu().tolist() == [0, 1, 0, 0]
    if group == "k_rows":                                                     # ids are row + idx_offset
        v2, i2, st2 = _raw(s.Qd, s.Dd, s.k, a, c, idx_offset=1000)
        assert torch.equal(v2, v) and torch.equal(i2, torch.where(i >= 0, i + 1000, i)) and torch.equal(st2, st)


def test_seven_rows_beside_an_unrestricted_neighbour(dev):
    s = _data("B4_N5000_d768", dev)
    a = _allowed(s, ("all", "seven_rows", "all", "two_percent"), 8192)
    v, i, st = _raw(s.Qd, s.Dd, s.k, a, 2)
    clean = _check(s, a, 8192, v, i, st, "N = 5000", strict=True)
    assert st.cpu().tolist() == [0, 0, 0, 0] and (i[1, 7:] == -1).all() and (i[1, :7] >= 0).all() and (i[0] >= 0).all()
    _check_against_exhaustive(s, a, i, clean)
    assert clean.sum() >= 2


@pytest.mark.parametrize("form,c", [("B40_d128", 2), ("B40_d128", 3), ("bf16_B40_d256", 2), ("B1_d128", 1)])
def test_a_batch_is_its_queries_one_by_one(dev, form, c):
    """Every filter of the module in one call, a different one per query; then oracle 2: row q is the one-query call's, bit for bit."""
    s = _data(form, dev)
    cap = gather_ref.cap_of(c)
    names = [f for f in FILTERS if c > 2 or f != "fifty_percent"] if s.B > 1 else ["two_percent"]
    a = _allowed(s, names, cap)
    v, i, st = _raw(s.Qd, s.Dd, s.k, a, c)
    clean = _check(s, a, cap, v, i, st, f"{form} / c = {c}")
    assert s.B == 1 or (st.sum() >= 1 and clean.sum() >= s.B // 4)
    _check_against_exhaustive(s, a, i, clean)
    for q in range(s.B):
        v1, i1, st1 = _raw(s.Qd[q:q + 1].contiguous(), s.Dd, s.k, a[q:q + 1], c)
        assert torch.equal(v1[0], v[q]) and torch.equal(i1[0], i[q]) and int(st1[0]) == int(st[q]), f"query {q} alone differs from its row of the batch"
    x = _raw(s.Qd, s.Dd, s.k, a, c)
    assert all(torch.equal(p, r) for p, r in zip(x, (v, i, st))), "two runs differ"


@pytest.mark.parametrize("k", [10, 1024])
def test_chunked_regime(dev, k):
    """N = 40 000 with 9 000 and 12 289 allowed rows at c = 4: three chunks, and four of which the last holds one position."""
    s = _data("chunked_B2", dev)
    rng = np.random.default_rng(5)
    a = np.zeros((2, s.N), bool)
    a[0, rng.choice(s.N, 9000, replace=False)] = True
    a[1, rng.choice(s.N, 12_289, replace=False)] = True
    v, i, st = _raw(s.Qd, s.Dd, k, a, 4)
    clean = _check(s, a, 16_384, v, i, st, f"chunked k = {k}", k=k)
    assert st.cpu().tolist() == [0, 0]
    _check_against_exhaustive(s, a, i, clean, k=k)
    v3, i3, st3 = _raw(s.Qd, s.Dd, k, a, 3)                                   # cap 12 288: query 1 loses its last row and is flagged
    _check(s, a, 12_288, v3, i3, st3, f"chunked k = {k}, c = 3", k=k)
    assert st3.cpu().tolist() == [0, 1] and torch.equal(v3[0], v[0]) and torch.equal(i3[0], i[0])


@pytest.mark.parametrize("k", [10, 1024])
def test_one_sort_and_chunks_give_the_same_bits(dev, k):
    """c = 2 (one LDS sort) against c = 3 (chunks plus a merge round) on the same <= 8 192 rows per query."""
    s = _data("chunked_B2", dev)
    rng = np.random.default_rng(6)
    a = np.zeros((2, s.N), bool)
    a[0, rng.choice(s.N, 8192, replace=False)] = True
    a[1, rng.choice(s.N, 4097, replace=False)] = True
    a[1, s.dups[1]] = True
    one, chunks = _raw(s.Qd, s.Dd, k, a, 2), _raw(s.Qd, s.Dd, k, a, 3)
    assert all(torch.equal(x, y) for x, y in zip(one, chunks)) and one[2].cpu().tolist() == [0, 0]
    _check(s, a, 8192, *one, f"one sort, k = {k}", k=k)


def test_every_row_allowed_takes_two_merge_rounds(dev):
    """N = 70 001, everything allowed, c = 18, k = 1024: 18 partial lists, 8 per merge workgroup -> 3 -> 1."""
    s = _data("all_rows_B2", dev)
    a = np.ones((2, s.N), bool)
    v, i, st = _raw(s.Qd, s.Dd, s.k, a, 18)
    clean = _check(s, a, 18 * 4096, v, i, st, "all rows")
    assert st.cpu().tolist() == [0, 0]
    _check_against_exhaustive(s, a, i, clean)


@pytest.mark.parametrize("form,c", [("B4_d132", 2), ("bf16_B4_d72", 1), ("chunked_B2", 3)])
def test_memory_contract_of_the_mode(dev, form, c):
    """A workspace of exactly the declared size between guard bands, the scratch behind the bitmaps poisoned, garbage in the ignored
    bits past N and in every bitmap's padding up to M and that region bit-identical after the call, guarded outputs, operands with
    winning rows behind them, a non-default stream, status = NULL, two runs."""
    s = _data(form, dev)
    cap = gather_ref.cap_of(c)
    a = _allowed(s, ("two_percent", "cap_plus_1", "ties", "row_last"), cap)
    M, W = live_ref.mask_bytes(s.N), (s.N + 31) // 32
    need = lib().gdr_sim_topk_workspace_bytes(s.B, s.N, s.d, s.k, _flags(c))
    assert need >= s.B * M + 8 * s.B * cap
    words = np.stack([live_ref.pack(r) for r in a])
    if s.N % 32:
        words[:, -1] |= np.int32(-1) << np.int32(s.N % 32)                   # bits past N: ignored
    region = torch.full((s.B, M), 0xA7, dtype=torch.uint8)                    # every bitmap's padding: ignored
    region[:, :W * 4] = torch.from_numpy(words.view(np.uint8).reshape(s.B, W * 4))
    region = region.reshape(-1).to(dev)
    far = torch.full((256, s.d), 10.0, dtype=s.Dd.dtype)                      # rows that would win every top-k if read
    Qd, qh = guarded_input(s.Qd.cpu(), tail=torch.full((128, s.d), 1e3, dtype=s.Qd.dtype))
    Dd, dh = guarded_input(s.Dd.cpu(), tail=far)
    fn = lib().gdr_sim_topk_bf16 if s.bf16 else lib().gdr_sim_topk
    side = torch.cuda.Stream(device=dev)
    runs = []
    for fill in (0x00, 0xFF, 0x5A):
        ws, hws = poisoned_workspace(need, fill, dev)
        ws[:s.B * M].copy_(region)
        v, hv = guarded((s.B, s.k), torch.float32, dev)
        i, hi = guarded((s.B, s.k), torch.int32, dev)
        st, hst = guarded((s.B,), torch.int32, dev)
        st_before = st.clone()
        side.wait_stream(torch.cuda.current_stream(dev))
        for rep in range(2 if fill == 0x5A else 1):                           # the last fill runs twice on the warm workspace
            null_status = fill == 0xFF
            with torch.cuda.stream(side):
                assert stream_ptr().value == side.cuda_stream and side.cuda_stream != 0
                rc = fn(ptr(Qd), s.B, ptr(Dd), s.N, s.d, s.k, 0, ptr(v), ptr(i), None if null_status else ptr(st), _flags(c), ptr(ws), need,
                        stream_ptr())
            assert rc == 0, lib().gdr_last_error().decode()
            side.synchronize()
            tag = f"{form} fill 0x{fill:02X} run {rep}"
            for h, name in ((hws, "workspace"), (hv, "out_val"), (hi, "out_idx"), (hst, "status")):
                h.check(f"{tag}: {name}")
            assert not null_status or torch.equal(st, st_before), f"{tag}: status = NULL, yet the caller's status buffer was written"
            assert torch.equal(ws[:s.B * M], region), f"{tag}: the bitmap region was written"
            runs.append((v.clone(), i.clone(), None if null_status else st.clone()))
    qh.unchanged("Q")
    dh.unchanged("D")
    assert lib().gdr_device_fault_pending() == 0
    for v, i, st in runs:
        assert torch.equal(v, runs[0][0]) and torch.equal(i, runs[0][1]), "the result depends on what the scratch held"
        assert st is None or torch.equal(st, runs[0][2])
    _check(s, a, cap, *runs[0], form)
    plain = _raw(s.Qd, s.Dd, s.k, a, c)                                       # the default stream, clean bitmaps
    assert all(torch.equal(x, y) for x, y in zip(plain, runs[0]))


def test_gather_call_in_a_captured_graph(dev):
    """ops.sim_topk(gather=8192, exact_on_overflow=False) returns a status and never synchronises: it is captured in a graph (a
    synchronisation would fail the capture), replayed, and replayed again after the QueryRows changed in place."""
    s = _data("B40_d128", dev)
    a = _allowed(s, [f for f in FILTERS if f != "fifty_percent"], 8192)
    R = ops.QueryRows.from_bool(torch.from_numpy(a).to(dev))
    need = lib().gdr_sim_topk_workspace_bytes(s.B, s.N, s.d, s.k, _flags(2))
    ws = live_ref.FixedWorkspace(torch.empty(need, dtype=torch.uint8, device=dev))
    call = lambda: ops.sim_topk(s.Qd, s.Dd, s.k, workspace=ws, allowed=R, gather=8192, exact_on_overflow=False, return_status=True)   # noqa: E731
    warm = torch.cuda.Stream(device=dev)
    warm.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(warm):
        ev, ei, est = call()                                                  # eager; also the one run a capture needs first
    torch.cuda.current_stream().wait_stream(warm)
    torch.cuda.synchronize()
    ev, ei, est = ev.clone(), ei.clone(), est.clone()
    _check(s, a, 8192, ev, ei, est, "eager")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gv, gi, gst = call()
    gv.zero_(), gi.zero_(), gst.fill_(-7)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(gv, ev) and torch.equal(gi, ei) and torch.equal(gst, est)
    got = ei.cpu().numpy()
    for q in range(s.B):                                                      # every query is now denied what it was just given
        a[q, got[q][got[q] >= 0]] = False
    R.words.copy_(ops.QueryRows.from_bool(torch.from_numpy(a).to(dev)).words)
    g.replay()
    torch.cuda.synchronize()
    after = gi.cpu().numpy()
    assert not any(np.isin(after[q][after[q] >= 0], got[q]).any() for q in range(s.B))
    _check(s, a, 8192, gv, gi, gst, "graph replay after the filters changed")


# ------------------------------------------------------------------------------------------------ the Python surface
def _spy(monkeypatch):
    calls, real = [], ops._sim_topk_raw

    def wrapped(Q, D, k, idx_offset, workspace, flags, live=None, allowed=None):
        calls.append(types.SimpleNamespace(Q=Q.clone(), flags=flags, live=live, allowed=allowed))
        return real(Q, D, k, idx_offset, workspace, flags, live, allowed)

    monkeypatch.setattr(ops, "_sim_topk_raw", wrapped)
    return calls


def _ref_check(s, a, v, i, what):
    _check(s, a, 2 ** 20, v, i, torch.zeros(s.B, dtype=torch.int32), what)


def test_mixed_batch_is_routed_by_row_count(dev, monkeypatch):
    """One 2 % query, one 7-row query and two unrestricted: gather="auto" sends exactly the two narrow ones through one gather call and
    the others through the dense masked call; no exhaustive re-run is made for the narrow ones.  gather=False (and the default of
    ops.sim_topk, None) issues the calls made before the mode existed: the dense call of all four, then the exhaustive re-run of the
    two that overflow."""
    s = _data("B4_N40000_d64", dev)
    assert s.N > ops.GATHER_MAX_ROWS
    a = _allowed(s, ("two_percent", "all", "seven_rows", "all"), 8192)
    R = ops.QueryRows.from_bool(torch.from_numpy(a).to(dev))
    calls = _spy(monkeypatch)
    v, i, st = ops.sim_topk(s.Qd, s.Dd, s.k, allowed=R, gather="auto", return_status=True)
    assert int(st.abs().sum()) == 0
    _ref_check(s, a, v, i, "auto")
    g = [c for c in calls if c.flags & RG]
    assert len(g) == 1 and torch.equal(g[0].Q, s.Qd[[0, 2]]) and g[0].flags & (0x1FF << 8) == _ffi.sim_gather_chunks(1)
    assert np.array_equal(g[0].allowed.to_bool().cpu().numpy(), a[[0, 2]])
    rest = [c for c in calls if not c.flags & RG]
    assert len(rest) == 1 and torch.equal(rest[0].Q, s.Qd[[1, 3]]) and not rest[0].flags & EXH
    for kw in ({"gather": False}, {}):
        del calls[:]
        fv, fi = ops.sim_topk(s.Qd, s.Dd, s.k, allowed=R, **kw)
        assert [(c.Q.shape[0], c.flags) for c in calls] == [(4, 0), (2, EXH)] and torch.equal(calls[1].Q, s.Qd[[0, 2]])
        _ref_check(s, a, fv, fi, "gather=False")
        assert torch.equal(fi, i)
    del calls[:]                                                              # an all-narrow batch launches no dense pass
    nv, ni = ops.sim_topk(s.Qd[[0, 2]].contiguous(), s.Dd, s.k, allowed=R.rows([0, 2]), gather="auto")
    assert len(calls) == 1 and calls[0].flags & RG and torch.equal(nv, v[[0, 2]]) and torch.equal(ni, i[[0, 2]])
    del calls[:]                                                              # no read-back without exact_on_overflow: "auto" is the dense call
    ops.sim_topk(s.Qd, s.Dd, s.k, allowed=R, gather="auto", exact_on_overflow=False)
    assert [(c.Q.shape[0], c.flags) for c in calls] == [(4, 0)]
    with pytest.raises(_ffi.GdrError, match="gather"):
        ops.sim_topk(s.Qd, s.Dd, s.k, gather=8192)
    with pytest.raises(_ffi.GdrError, match="gather"):
        ops.sim_topk(s.Qd, s.Dd, s.k, allowed=R, gather=True)


def test_auto_route_sizes_one_gather_call_for_its_longest_narrow_list(dev, monkeypatch):
    """12 289 rows beside 2 %, an unrestricted query and 7 rows: the three narrow ones share one call of 4 chunks (the chunked regime),
    the unrestricted one takes the dense call alone."""
    s = _data("B4_N40000_d64", dev)
    assert 12_289 <= ops.GATHER_MAX_ROWS < s.N
    a = _allowed(s, ("cap_plus_1", "two_percent", "all", "seven_rows"), 12_288)
    calls = _spy(monkeypatch)
    v, i = ops.sim_topk(s.Qd, s.Dd, s.k, allowed=ops.QueryRows.from_bool(torch.from_numpy(a).to(dev)), gather="auto")
    assert [(c.Q.shape[0], bool(c.flags & RG), c.flags & (0x1FF << 8)) for c in calls] == [(3, True, _ffi.sim_gather_chunks(4)), (1, False, 0)]
    assert torch.equal(calls[0].Q, s.Qd[[0, 1, 3]]) and torch.equal(calls[1].Q, s.Qd[[2]])
    _ref_check(s, a, v, i, "auto, chunked")


def test_forced_gather_flags_what_it_cannot_hold_and_the_default_repairs_it(dev):
    s = _data("B4_d128", dev)
    a = _allowed(s, ("two_percent", "cap_plus_1", "seven_rows", "fifty_percent"), 4096)
    R = ops.QueryRows.from_bool(torch.from_numpy(a).to(dev))
    v, i, st = ops.sim_topk(s.Qd, s.Dd, s.k, allowed=R, gather=4096, exact_on_overflow=False, return_status=True)
    assert st.cpu().tolist() == [0, 1, 0, 1]
    _check(s, a, 4096, v, i, st, "gather=4096")
    ev, ei, est = ops.sim_topk(s.Qd, s.Dd, s.k, allowed=R, gather=4096, return_status=True)
    assert int(est.abs().sum()) == 0 and torch.equal(ev[[0, 2]], v[[0, 2]]) and torch.equal(ei[[0, 2]], i[[0, 2]])
    _ref_check(s, a, ev, ei, "gather=4096, exact")


def test_live_and_allowed_together_are_their_and(dev):
    s = _data("B40_d128", dev)
    a = _allowed(s, [f for f in FILTERS if f != "cap_plus_1"], 8192)
    live = np.random.default_rng(21).random(s.N) < 0.8
    L = ops.LiveRows.from_bool(torch.from_numpy(live).to(dev))
    R = ops.QueryRows.from_bool(torch.from_numpy(a).to(dev))
    for kw in ({"gather": 8192}, {"gather": "auto"}):
        bv, bi = ops.sim_topk(s.Qd, s.Dd, s.k, live=L, allowed=R, **kw)
        assert np.array_equal(R.to_bool().cpu().numpy(), a), "sim_topk must not change the caller's QueryRows"
        both = R.rows(torch.arange(s.B)).and_(L)
        av, ai = ops.sim_topk(s.Qd, s.Dd, s.k, allowed=both, **kw)
        assert torch.equal(bv, av) and torch.equal(bi, ai)
        _ref_check(s, a & live, bv, bi, f"live= and allowed=, {kw}")
    pv, pi = ops.sim_topk(s.Qd, ops.PrefilteredCorpus(s.Dd), s.k, allowed=both, gather="auto")   # searched through .D
    assert torch.equal(pv, av) and torch.equal(pi, ai)


def _args(V, R=4):
    return types.SimpleNamespace(num_return_sequences=R, output_vocab_size=V, max_output_length=4, length_penalty=0.8, kary=V,
                                 position=1, score_rate=[0, 1.0], loss_func="tanh")


def test_retriever_search_with_a_filter_after_remove_documents(dev, monkeypatch):
    """GDRRetriever.search(allowed=) routes by default: every query's filter is narrow here, so one gather call serves the batch, and a
    removed document that a filter allows does not come back."""
    from gdr_amd.modeling import DenseModel, GDRRetriever
    V, csz, d, k, B = 30, 3, 64, 20, 6
    names = ["-".join(str(x) for x in synth.cluster_digits(c, 2, V)) for c in range(V * V)]
    N = len(names) * csz
    D0 = synth.make_corpus(N, d, cluster_size=csz, seed=8)
    Q, _ = synth.make_queries(D0, B, seed=3)
    Qd = torch.from_numpy(Q).to(dev)
    idx = codec.ClusterIndex(names, (np.arange(len(names) + 1) * csz).astype(np.int32), np.arange(N, dtype=np.int32))
    r = GDRRetriever(None, torch.from_numpy(D0).to(dev), idx, _args(V))
    base = r.search(Qd, k)[1].cpu().numpy()
    gone = np.unique(np.concatenate([base[:, :5].reshape(-1), np.arange(0, N, 7)]))
    offs, mem, n = lifecycle_ref.remove(idx.offsets, idx.members, gone)
    assert r.remove_documents(gone) == n
    live = np.zeros(N, bool)
    live[np.asarray(mem)] = True
    a = np.random.default_rng(4).random((B, N)) < 0.5
    for q in range(B):
        a[q, base[q, :10]] = True                                             # allowed by the filter; the first five are removed
    R = ops.QueryRows.from_bool(torch.from_numpy(a).to(dev))
    calls = _spy(monkeypatch)
    v, i = r.search(Qd, k, allowed=R)
    assert len(calls) == 1 and calls[0].flags & RG and calls[0].Q.shape[0] == B
    assert i.dtype == torch.int64 and np.array_equal(R.to_bool().cpu().numpy(), a)
    assert not np.isin(i.cpu().numpy(), gone).any(), "a removed document that the filter allows came back"
    s = types.SimpleNamespace(S=live_ref.scores(Q, D0), B=B, N=N, k=k)
    _ref_check(s, a & live, v, i.to(torch.int32), "GDRRetriever.search(allowed=)")
    L = ops.LiveRows.from_bool(torch.from_numpy(live).to(dev))
    fv, fi = DenseModel(None).search(Qd, r.doc_embed, k, live=L, allowed=R)
    assert torch.equal(v, fv) and torch.equal(i, fi)
    dv, di = r.search(Qd, k, allowed=R, gather=False)                         # the dense masked call: the same documents
    _ref_check(s, a & live, dv, di.to(torch.int32), "GDRRetriever.search(allowed=, gather=False)")
    sh = GDRRetriever(None, r.doc_embed, r.index, _args(V), sharded=types.SimpleNamespace(D=r.doc_embed))
    with pytest.raises(_ffi.GdrError, match="sharded"):
        sh.search(Qd, k, allowed=R)
