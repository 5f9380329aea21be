"""Row-scaled entry points on operands of more than 2^31 elements / 4 GiB: the corpus kernels (`D + row * d`), the corpus-wide
helpers and the linears whose A, C or plane buffers cross the boundary.  Everything else in the suite stays far below 2^31
elements, so a single 32-bit product in an address expression would pass it; here such a product reads another row (a plausible,
wrong score) or faults.

Shapes (the smallest that cross): d = 768 puts element 2^31 into row R31 = 2 796 202 (it straddles: the row starts 512 elements
before it) and, for fp32, byte 2^32 into row R32B = 1 398 101; for the bf16 image byte 2^32 lies in row R31.  The corpus has
N = 2 800 003 rows (odd, no multiple of a tile, 3 801 rows at or past R31).  The linears take M = 700 001 rows: with a leading
dimension of 3072 element 2^31 lies in row 699 050 and fp32 byte 2^32 in row 349 525.

Operands are drawn on the device from seeded generators, in row chunks.  References are plain torch on the device (independent of
the library): float64 over the whole tensor where that is cheap, otherwise torch's fp32 over the whole tensor plus float64 over
the WINDOWS — rows [0, 256), 128 rows on either side of every boundary row, the 256 rows before the last 200, the last 200.

Planted documents (similarity).  Query b owns 8 rows holding c_j * q_b with 8 distinct c_j in [1.5, 2.5]: scores ~ 768 c_j against
a random maximum of ~150, so they lead its top-k in a known order.  One row cannot be a multiple of 40 different queries, so only
query 0 owns the boundary rows themselves (R32B-1, R32B, R32B+1, R31-1, R31, R31+1, N-2, row 1000); query b owns their nearest
free neighbours on the same side of each boundary (R32B-1-b, R32B+2b, R32B+2b+1, R31-1-b, R31+2b, R31+2b+1, N-2-b, 1000+b).
The pre-filter's asserted run uses a copy of the corpus whose planted rows are scaled by 0.4 (c_j in [0.6, 1.0], scores 420 .. 840,
still three times the random maximum).  Its band is 2 eps_q = 2 |q| max|D[r]| (2^-7 + ...) wide: a planted row of norm 2.5 |q| widens
it from ~14 to ~31 score units around the 100-th score (~110), thousands of documents where gdr_sim_topk_prefilter holds 1 024, so
over the unscaled corpus every status is 1 by the header's contract — an overflow of the band, not of an address.  That corpus is
run too: the flags must be raised, and the repaired result (ops.sim_topk's default, the exhaustive fp32 pass over the flagged
queries) must hold the planted ids and the fp32 reference.

Not here: gdr_kmeans_partition, gdr_cluster_insert and gdr_topk_merge* index int32 ids and lists of at most 2^31 entries of 4 or 8
bytes; none of their operands can cross either boundary at these sizes.  The encoder / doc-tower / generate entry points batch
below 2^31 elements.

Live device memory stays below 40 GB (asserted after every test from the allocator's peak): the corpus (12.9 GB with its bf16
image) and the linear operands live in _CACHE alone — tests fetch them with _corpus(dev) / _linear_operands(dev) and keep no
reference — and each group drops the other's entry, and checks that the memory came back, before it allocates."""
import gc

import numpy as np
import pytest
import torch

from gdr_amd import _ffi, ops
from gdr_amd._ffi import lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL = 1e-4                       # fp32 scores abs(d) <= 1e-4 + 1e-4 * abs(ref)
D_MODEL = 768
N_DOCS = 2_800_003
R31 = 2_796_202                  # the row of element 2^31 (and of byte 2^32 of the bf16 image)
R32B = 1_398_101                 # the row of byte 2^32 of the fp32 image
M_ROWS = 700_001
LD = 3072
M31 = 699_050                    # ld = 3072: the row of element 2^31
M32B = 349_525                   # ... and of fp32 byte 2^32
STREAMK_BYTES = _ffi.STREAMK_WS_BYTES
MEM_LIMIT = 40 * 10 ** 9         # live device memory of this module, at any moment
K_TOP, B_MAX = 100, 40
PLANT_C = np.linspace(2.5, 1.5, 8)
PREFILTER_PLANT_SCALE = 0.4


def test_the_boundary_rows_are_where_the_docstring_says():
    assert R31 == 2 ** 31 // D_MODEL and 2 ** 31 - R31 * D_MODEL == 512 and R32B == 2 ** 32 // (4 * D_MODEL)
    assert (N_DOCS - 1) * D_MODEL >= 2 ** 31 and N_DOCS - R31 == 3801 and N_DOCS % 2 == 1 and all(N_DOCS % t for t in (32, 64, 128, 256))
    assert M31 == 2 ** 31 // LD and M32B == 2 ** 32 // (4 * LD) and M_ROWS * LD >= 2 ** 31 and M_ROWS * 1536 * 2 >= 2 ** 31


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


# ================================================================================================ plumbing
_CACHE = {}                      # "corpus" / "linear": the big operands of one group; a group drops the other's before it allocates


def _drop(*groups):
    for g in groups:
        _CACHE.pop(g, None)
    gc.collect()
    torch.cuda.empty_cache()


def _assert_released(what):
    """After a group was dropped nothing big may be left: the other group's operands would otherwise live beside the new ones."""
    torch.cuda.synchronize()
    gc.collect()
    live = torch.cuda.memory_allocated()
    assert live < 1 << 30, f"{what}: {live} bytes are still allocated after the other group was dropped"


@pytest.fixture(autouse=True)
def _live_memory_stays_below_40_gb():
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    yield
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    assert peak < MEM_LIMIT, f"peak live device memory {peak} bytes"


@pytest.fixture(scope="module", autouse=True)
def _release_everything_at_the_end():
    yield
    _drop("corpus", "linear")


def _need(dev, nbytes, what):
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info(dev)
    if free < nbytes:
        pytest.skip(f"{what}: needs {nbytes} bytes of device memory, {free} of {total} are free")


def _randn(rows, cols, seed, dev, scale=1.0, chunk=1 << 18):
    """fp32 [rows, cols] ~ N(0, scale^2), drawn on the device in row chunks from one seeded generator."""
    g = torch.Generator(device=dev).manual_seed(seed)
    out = torch.empty((rows, cols), dtype=torch.float32, device=dev)
    for lo in range(0, rows, chunk):
        out[lo:lo + chunk].normal_(0.0, scale, generator=g)
    return out


def _chunks(rows, chunk):
    return [(lo, min(lo + chunk, rows)) for lo in range(0, rows, chunk)]


def _windows(rows, boundaries, dev):
    parts = [torch.arange(0, 256)] + [torch.arange(b - 128, b + 128) for b in boundaries]
    parts += [torch.arange(rows - 456, rows - 200), torch.arange(rows - 200, rows)]
    w = torch.unique(torch.cat(parts))
    assert int(w.min()) == 0 and int(w.max()) == rows - 1
    return w.to(dev)


def _same_bits(a, b, chunk=1 << 18):
    """Bit equality of two big 2-D tensors, row chunk by row chunk (no whole-tensor temporary)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return all(torch.equal(a[lo:hi].view(it), b[lo:hi].view(it)) for lo, hi in _chunks(a.shape[0], chunk))


def _check(rc, what):
    assert rc == 0, f"{what}: rc {rc}: {lib().gdr_last_error().decode()}"


def _no_fault(what):
    torch.cuda.synchronize()
    assert lib().gdr_device_fault_pending() == 0, f"{what}: {lib().gdr_last_error().decode()}"


# ================================================================================================ the corpus
def _planted_rows(b):
    return [R32B - 1 - b, R32B + 2 * b, R32B + 2 * b + 1, R31 - 1 - b, R31 + 2 * b, R31 + 2 * b + 1, N_DOCS - 2 - b, 1000 + b]


def _planted_c(b):
    return np.roll(PLANT_C, b)                               # another order of the 8 factors for every query


def _reference_scores(Q64, rows_of, chunk=1 << 17):
    """float64 Q @ D^T over the whole corpus [B, N] (torch.topk follows).  rows_of(lo, hi) -> that row chunk as the kernel sees it."""
    S = torch.empty((Q64.shape[0], N_DOCS), dtype=torch.float64, device=Q64.device)
    for lo, hi in _chunks(N_DOCS, chunk):
        S[:, lo:hi] = Q64 @ rows_of(lo, hi).double().T
    return S


def _corpus(dev):
    """D fp32 [N, 768] with the planted rows, Q fp32 [40, 768], PrefilteredCorpus(D) (the bf16 image and the norm bound, made by
    the library), and the float64 references of the top-100: of the fp32 operands, of the bf16-rounded operands, and of the fp32
    operands with the planted rows scaled for the pre-filter."""
    if "corpus" in _CACHE:
        return _CACHE["corpus"]
    _drop("linear")
    _assert_released("corpus")
    _need(dev, 16 << 30, "corpus fixture (8.6 GB fp32 + 4.3 GB bf16 + references)")
    D = _randn(N_DOCS, D_MODEL, 20260101, dev)
    Q = _randn(B_MAX, D_MODEL, 20260102, dev)
    rows = torch.tensor([_planted_rows(b) for b in range(B_MAX)], device=dev)                  # [40, 8]
    cs = torch.tensor(np.stack([_planted_c(b) for b in range(B_MAX)]), dtype=torch.float32, device=dev)
    assert rows.unique().numel() == rows.numel() and int(rows.min()) >= 0 and int(rows.max()) < N_DOCS
    D[rows.view(-1)] = (cs.view(-1, 1) * Q.repeat_interleave(8, 0))
    expect = torch.gather(rows, 1, torch.argsort(cs, 1, descending=True)).cpu().numpy()        # planted ids, best first
    P = ops.PrefilteredCorpus(D)
    c = dict(D=D, Q=Q, P=P, rows=rows, expect=expect)
    Q64 = Q.double()
    S = _reference_scores(Q64, lambda lo, hi: D[lo:hi])
    c["ref_f32"] = tuple(t.cpu().numpy() for t in torch.topk(S, K_TOP, dim=1))
    flat = rows.view(-1)
    Dpf = D[flat] * PREFILTER_PLANT_SCALE                                                       # what _prefilter_corpus plants
    S[:, flat] = Q64 @ Dpf.double().T
    c["ref_prefilter"] = tuple(t.cpu().numpy() for t in torch.topk(S, K_TOP, dim=1))
    del S
    S = _reference_scores(Q.bfloat16().double(), lambda lo, hi: D[lo:hi].bfloat16())       # torch's rounding, not the library's
    c["ref_bf16"] = tuple(t.cpu().numpy() for t in torch.topk(S, K_TOP, dim=1))
    del S
    _CACHE["corpus"] = c
    return c


@pytest.fixture
def corpus(dev):
    """Function-scoped on purpose: pytest keeps a fixture's value until the end of its scope, and a module-scoped one would hold
    the 12.9 GB through the linear tests.  _CACHE is the only owner between tests."""
    return _corpus(dev)


def test_the_references_alone_rank_the_planted_rows_first_and_reach_past_4gib(corpus):
    """Before any kernel runs: in all three references the 8 planted rows of a query lead in the planned order and outscore the
    ninth entry at least twofold, and at least a third of every top-100 lies past row R32B."""
    for name in ("ref_f32", "ref_bf16", "ref_prefilter"):
        rv, ri = corpus[name]
        assert np.array_equal(ri[:, :8], corpus["expect"]), name
        margin = rv[:, 7] / rv[:, 8]
        past = (ri >= R32B).mean(1)
        print(f"{name}: planted scores {rv[:, 7].min():.0f} .. {rv[:, 0].max():.0f}, ninth <= {rv[:, 8].max():.0f}, margin >= {margin.min():.2f}; "
              f"share of the top-{K_TOP} past R32B {past.min():.2f} .. {past.max():.2f}, past R31 {(ri >= R31).sum(1).min()} .. {(ri >= R31).sum(1).max()} ids")
        assert margin.min() > 2.0, name
        assert (np.diff(rv[:, :8], axis=1) < -20.0).all(), name
        assert past.min() >= 1.0 / 3.0, name


def _sim_case(corpus, target, ref, B):
    from conftest import order_insensitive_topk_match
    v, i, st = ops.sim_topk(corpus["Q"][:B], target, K_TOP, return_status=True, exact_on_overflow=False)
    _no_fault("sim_topk")
    assert int(st.abs().sum()) == 0, f"status {st.cpu().tolist()}"
    v, i = v.cpu().numpy(), i.cpu().numpy().astype(np.int64)
    assert i.min() >= 0 and i.max() < N_DOCS
    assert np.array_equal(i[:, :8], corpus["expect"][:B]), "the planted documents are not found exactly and in order"
    rv, ri = corpus[ref]
    order_insensitive_topk_match(rv[:B], ri[:B], v, i, TOL)
    assert (np.diff(v, axis=1) <= 0).all()


@pytest.mark.parametrize("B", [8, B_MAX], ids=["stream_B8", "tiled_B40"])
@pytest.mark.parametrize("form", ["f32", "bf16"])
def test_sim_topk_over_a_corpus_past_2_31_elements(corpus, form, B):
    """gdr_sim_topk / gdr_sim_topk_bf16, k = 100: B = 8 takes the latency-mode stream kernels (sim_stream.hip), B = 40 the tiled
    core (gemm_f32.hip / gemm_bf16.hip)."""
    target = corpus["D"] if form == "f32" else corpus["P"].D16
    _sim_case(corpus, target, "ref_" + form, B)


def _prefilter_corpus(corpus):
    D2 = corpus["D"].clone()
    flat = corpus["rows"].view(-1)
    D2[flat] = D2[flat] * PREFILTER_PLANT_SCALE
    return ops.PrefilteredCorpus(D2)


@pytest.mark.parametrize("B", [8, B_MAX], ids=["stream_B8", "tiled_B40"])
def test_sim_topk_prefilter_over_a_corpus_past_2_31_elements(dev, corpus, B):
    """gdr_sim_topk_prefilter: the bf16 pass streams the image (byte 2^32 in row R31), the tail gathers fp32 rows by id (byte 2^32
    in row R32B).  Asserted clean on the corpus with the planted rows scaled by 0.4; over the unscaled rows (module docstring) the
    band must be flagged as overflowed, and the repaired result must be the fp32 reference with the planted ids in front."""
    from conftest import order_insensitive_topk_match
    _need(dev, 15 << 30, "a second corpus for the pre-filter (8.6 GB fp32 + 4.3 GB bf16)")
    _v, _i, st = ops.sim_topk(corpus["Q"][:B], corpus["P"], K_TOP, return_status=True, exact_on_overflow=False)
    print(f"pre-filter over the unscaled planted rows (dnorm_max {corpus['P'].dnorm_max:.1f}): {int((st != 0).sum())} of {B} queries flag an overflowed band")
    assert int((st != 0).sum()) == B, "a band of thousands of documents must be reported, not cut silently"
    v, i, st = ops.sim_topk(corpus["Q"][:B], corpus["P"], K_TOP, return_status=True)        # exact_on_overflow: the exhaustive fp32 repair
    _no_fault("sim_topk repair")
    assert int(st.abs().sum()) == 0
    v, i = v.cpu().numpy(), i.cpu().numpy().astype(np.int64)
    assert np.array_equal(i[:, :8], corpus["expect"][:B]), "the repaired lists do not start with the planted documents"
    order_insensitive_topk_match(corpus["ref_f32"][0][:B], corpus["ref_f32"][1][:B], v, i, TOL)
    del _v, _i, v, i, st
    _drop()
    P2 = _prefilter_corpus(corpus)
    try:
        assert P2.dnorm_max < 33.0, P2.dnorm_max                 # the planted rows do not set the norm bound
        _sim_case(corpus, P2, "ref_prefilter", B)
    finally:
        del P2
        _drop()


# ------------------------------------------------------------------------------------------------ corpus-wide helpers
def test_cast_f32_bf16_whole_corpus(dev, corpus):
    D = corpus["D"]
    assert D.numel() >= 2 ** 31
    out = ops.to_bf16(D)
    _no_fault("cast")
    for lo, hi in _chunks(N_DOCS, 1 << 18):
        assert torch.equal(out[lo:hi], D[lo:hi].bfloat16()), f"rows [{lo}, {hi})"
    assert _same_bits(out, corpus["P"].D16)


def test_row_norm2_max_finds_the_largest_row_at_the_end_and_at_2_31(dev, corpus):
    D = corpus["D"]
    n2 = torch.cat([(D[lo:hi].double() ** 2).sum(1) for lo, hi in _chunks(N_DOCS, 1 << 18)])
    out = torch.empty(1, dtype=torch.float32, device=dev)
    for row in (N_DOCS - 1, R31):
        keep = D[row].clone()
        try:
            D[row] = _randn(1, D_MODEL, row, dev, scale=4.0)[0]                  # norm^2 ~ 12 000 against <= ~5 000 elsewhere
            ref = n2.clone()
            ref[row] = (D[row].double() ** 2).sum()
            assert int(ref.argmax()) == row and float(ref[row]) > 1.5 * float(n2.max())
            _check(lib().gdr_row_norm2_max(ptr(D), N_DOCS, D_MODEL, ptr(out), stream_ptr()), "gdr_row_norm2_max")
            _no_fault("row_norm2_max")
            want = float(ref.max())
            assert abs(float(out[0]) - want) <= 1e-5 * want, (row, float(out[0]), want)
        finally:
            D[row] = keep


@pytest.mark.parametrize("op", ["l2_normalize", "t5_layer_norm"])
def test_row_norms_over_the_whole_corpus_in_place_and_out_of_place(dev, corpus, op):
    _need(dev, 18 << 30, "two [N, 768] fp32 results")
    D = corpus["D"]
    w = _randn(1, D_MODEL, 77, dev)[0]
    if op == "l2_normalize":
        fn = lambda src, dst: lib().gdr_l2_normalize(ptr(src), ptr(dst), N_DOCS, D_MODEL, 1e-12, stream_ptr())      # noqa: E731
        ref = lambda x: x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)                                             # noqa: E731
    else:
        fn = lambda src, dst: lib().gdr_t5_layer_norm(ptr(src), ptr(w), ptr(dst), N_DOCS, D_MODEL, 1e-6, stream_ptr())   # noqa: E731
        ref = lambda x: w.double() * (x / torch.sqrt((x * x).mean(-1, keepdim=True) + 1e-6))                          # noqa: E731
    out = torch.empty_like(D)
    _check(fn(D, out), op)
    inp = D.clone()
    _check(fn(inp, inp), op + " in place")
    _no_fault(op)
    assert _same_bits(out, inp), f"{op}: in place differs from out of place"
    del inp
    for lo, hi in _chunks(N_DOCS, 1 << 17):
        # fp32 against float64: a handful of roundings of 2^-24 each (tests/test_gpu_abi_memory.py)
        torch.testing.assert_close(out[lo:hi].double(), ref(D[lo:hi].double()), rtol=2e-6, atol=1e-7, msg=lambda m: f"{op} rows [{lo}, {hi}): {m}")
    del out
    _drop()


# ------------------------------------------------------------------------------------------------ gathers by id
def _gather_ids(rng, n):
    """n distinct doc ids in random order: half at or past R31, a quarter in [R32B, R31), a quarter below; R31 and N - 1 themselves
    come first, so that every prefix holds them."""
    hi = rng.choice(np.arange(R31 + 1, N_DOCS - 1), n // 2 - 2, replace=False)
    mid = rng.choice(np.arange(R32B, R31), n // 4, replace=False)
    lo = rng.choice(R32B, n - n // 2 - n // 4, replace=False)
    ids = np.concatenate([[R31, N_DOCS - 1], rng.permutation(np.concatenate([hi, mid, lo]))]).astype(np.int32)
    assert len(set(ids.tolist())) == n and (ids >= R31).sum() == n // 2
    return ids


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("func", ["tanh", "sigmoid"])
def test_rerank_gathers_rows_past_2_31_elements(dev, corpus, bf16, func):
    from conftest import ranked_lists_match
    from oracle import retrieval_ref
    rng = np.random.default_rng(31)
    B, R, k = 4, 5, 10
    alphas = [0, 0.5, 1, 3]
    ids = _gather_ids(rng, 256)
    sizes = rng.integers(9, 16, B * R)
    assert sizes.sum() <= len(ids)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    cand = ids[:offs[-1]].copy()
    cand[1], cand[offs[7]] = cand[offs[7]], cand[1]                               # row N - 1 moves to the second query
    assert cand[0] == R31 and cand[offs[7]] == N_DOCS - 1 and (cand >= R31).sum() > 60
    Dsrc = corpus["P"].D16 if bf16 else corpus["D"]
    q = _randn(B, D_MODEL, 5, dev, scale=0.03)                                    # away from tanh / sigmoid saturation
    beam = np.sort(rng.standard_normal((B, R)).astype(np.float32) * 2 - 8, axis=1)[:, ::-1].copy()
    max_cand = int(max(offs[(b + 1) * R] - offs[b * R] for b in range(B)))
    v, i = ops.rerank_topk(q, Dsrc, torch.from_numpy(offs).to(dev), torch.from_numpy(cand).to(dev), torch.from_numpy(beam).to(dev), alphas, k,
                           func=func, max_cand=max_cand)
    _no_fault("rerank")
    v, i = v.cpu().numpy(), i.cpu().numpy()
    uniq, local = np.unique(cand, return_inverse=True)
    Dg = Dsrc[torch.from_numpy(uniq.astype(np.int64)).to(dev)].float().cpu()      # the gathered rows (bf16: widened exactly), by torch
    qc = q.cpu()
    for b in range(B):
        lo, hi = offs[b * R], offs[(b + 1) * R]
        ref = retrieval_ref.rerank(qc[b:b + 1], Dg, [local[lo:hi].tolist()], [sizes[b * R:(b + 1) * R].tolist()], beam[b:b + 1].tolist(),
                                   alphas, k, func=func)[0]
        for a in range(len(alphas)):
            rv, ri = ref[a]
            np.testing.assert_allclose(v[b, a], rv.numpy(), rtol=TOL, atol=TOL)
            ranked_lists_match(uniq[ri.numpy()].tolist(), rv.numpy(), i[b, a].tolist(), TOL)


def test_cluster_centroids_gather_rows_past_2_31_elements(dev, corpus):
    import expand_ref
    rng = np.random.default_rng(32)
    ids = _gather_ids(rng, 400)
    sizes = [12, 0, 1, 40, 13, 11, 9, 100, 12, 12]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    mem = np.concatenate([np.sort(ids[offs[c]:offs[c + 1]]) for c in range(len(sizes))]).astype(np.int32)
    assert R31 in mem and N_DOCS - 1 in mem
    assert all(np.all(np.diff(mem[offs[c]:offs[c + 1]]) > 0) for c in range(len(sizes))) and (mem >= R31).sum() > 50
    cent, counts = ops.cluster_centroids_csr(corpus["D"], torch.from_numpy(offs).to(dev), torch.from_numpy(mem).to(dev))
    _no_fault("cluster_centroids")
    uniq, local = np.unique(mem, return_inverse=True)
    Dg = corpus["D"][torch.from_numpy(uniq.astype(np.int64)).to(dev)].cpu().numpy()
    rc, rn = expand_ref.centroids(Dg, offs, local.astype(np.int32))              # ascending ids stay ascending after the remap
    assert np.array_equal(counts.cpu().numpy(), rn)
    assert np.array_equal(cent.cpu().numpy().view(np.uint32), rc.view(np.uint32)), "centroids not bit-identical to the restatement"


def test_kmeans_assign_and_update_gather_rows_past_2_31_elements(dev, corpus):
    """One level with four nodes, d = 768, k = 30: the band rule of test_every_row_of_a_768_wide_round_is_within_the_fp32_band for
    every row, and the update bit-identical to the two-stage restatement (tests/kmeans_ref.py), on the gathered rows."""
    import kmeans_ref as kr
    rng = np.random.default_rng(33)
    d, k = D_MODEL, 30
    sizes = [700, 31, 300, 129]
    ids = _gather_ids(rng, sum(sizes))
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    rows = np.concatenate([np.sort(ids[off[s]:off[s + 1]]) for s in range(len(sizes))]).astype(np.int32)
    assert R31 in rows and N_DOCS - 1 in rows and (rows >= R31).sum() == len(rows) // 2
    uniq, local = np.unique(rows, return_inverse=True)
    X = corpus["D"][torch.from_numpy(uniq.astype(np.int64)).to(dev)].cpu().numpy()         # gathered by torch
    cent = np.concatenate([X[rng.choice(local[off[s]:off[s + 1]], k, replace=False)] for s in range(len(sizes))])
    rows_d, off_d = torch.from_numpy(rows).to(dev), torch.from_numpy(off).to(dev)
    lab, sc, ch, st = ops.kmeans_assign(corpus["D"], rows_d, off_d, torch.from_numpy(cent).to(dev), k)
    _no_fault("kmeans_assign")
    assert int(st.item()) == 0 and ch.cpu().tolist() == sizes
    lab_h, sc_h = lab.cpu().numpy(), sc.cpu().numpy()
    assert lab_h.min() >= 0 and lab_h.max() < k
    X64 = X.astype(np.float64)
    for s in range(len(sizes)):
        p = slice(off[s], off[s + 1])
        Xs, C64 = X64[local[p]], cent[s * k:(s + 1) * k].astype(np.float64)
        score = Xs @ C64.T - 0.5 * (C64 * C64).sum(1)[None, :]
        band = (2 * d + 8) * 2.0 ** -24 * np.linalg.norm(Xs, axis=1) * np.linalg.norm(C64, axis=1).max()
        chosen = score[np.arange(sizes[s]), lab_h[p]]
        assert (score.max(1) - chosen <= band).all(), f"node {s}: a row chose a centroid outside the fp32 band"
        assert (np.abs(sc_h[p] - chosen) <= band).all(), f"node {s}: a score outside the fp32 band"
    crow, coff, pst = ops.kmeans_partition(rows_d, lab, off_d, k)
    assert int(pst.item()) == 0
    c2, n2 = ops.kmeans_centroids(corpus["D"], coff, crow)
    _no_fault("kmeans_centroids")
    crow_h, coff_h, c2, n2 = crow.cpu().numpy(), coff.cpu().numpy(), c2.cpu().numpy(), n2.cpu().numpy()
    pos = {int(r): j for j, r in enumerate(uniq)}
    assert np.array_equal(n2, np.diff(coff_h)) and n2.sum() == len(rows)
    for c in range(len(sizes) * k):
        m = crow_h[coff_h[c]:coff_h[c + 1]]
        if len(m) == 0:
            assert not c2[c].any()
            continue
        want = kr.two_stage_mean(X, [pos[int(r)] for r in m])
        assert np.array_equal(c2[c].view(np.uint32), want.view(np.uint32)), f"child {c} ({len(m)} members)"


# ================================================================================================ linears
F = dict(PERSISTENT=_ffi.F32_FORM_PERSISTENT, STREAMK_TAIL=_ffi.F32_FORM_STREAMK_TAIL)
M_BELOW = 699_000                # M * 3072 < 0x7fffffff <= 700 001 * 3072
EPI_CASES = [("none", _ffi.EPI_NONE), ("bias_residual_in_place", _ffi.EPI_BIAS_RESIDUAL)]


def _linear_operands(dev):
    """A fp32 [700 001, 3072] (8.6 GB), shared by every linear case: its first columns / rows serve the smaller shapes."""
    if "linear" in _CACHE:
        return _CACHE["linear"]
    _drop("corpus")
    _assert_released("linear operands")
    _need(dev, 30 << 30, "linear operands and results (A 8.6 GB beside R, C and a reference chunk)")
    A = _randn(M_ROWS, LD, 20260201, dev)
    ws = torch.empty(STREAMK_BYTES, dtype=torch.uint8, device=dev)
    _CACHE["linear"] = dict(A=A, ws=ws)
    return _CACHE["linear"]


def _f32_linear(A, lda, W, C_, ldc, M, N, K, epi, bias, res, ldr, ws):
    if ws is None:
        rc = lib().gdr_linear_f32(ptr(A), lda, ptr(W), W.shape[1], ptr(C_), ldc, M, N, K, epi, ptr(bias), ptr(res), ldr, stream_ptr())
    else:
        rc = lib().gdr_linear_f32_splitk(ptr(A), lda, ptr(W), W.shape[1], ptr(C_), ldc, M, N, K, epi, ptr(bias), ptr(res), ldr, ptr(ws), ws.numel(),
                                         stream_ptr())
    _check(rc, f"linear {M} x {N} x {K}")


def _check_linear(out, a_of, W, bias, res_of, M, win, what):
    """out [M, N] against torch: the whole tensor against the fp32 matmul on the device, the windows against float64, both at TOL.
    a_of(rows) / res_of(rows) -> the operand rows as the kernel saw them (rows: a slice or an index tensor); res_of may be None."""
    Wt = W.float().T.contiguous()
    for lo, hi in _chunks(M, min(1 << 16, (1 << 26) // W.shape[0])):             # temporaries of at most 256 MB / 800 MB (an A chunk)
        ref = a_of(slice(lo, hi)).float() @ Wt
        if bias is not None:
            ref += bias
        if res_of is not None:
            ref += res_of(slice(lo, hi))
        torch.testing.assert_close(out[lo:hi], ref, rtol=TOL, atol=TOL, msg=lambda m: f"{what} rows [{lo}, {hi}) against fp32: {m}")
    ref = a_of(win).double() @ W.double().T
    if bias is not None:
        ref += bias.double()
    if res_of is not None:
        ref += res_of(win).double()
    torch.testing.assert_close(out[win].double(), ref, rtol=TOL, atol=TOL, msg=lambda m: f"{what} windows against float64: {m}")


@pytest.mark.parametrize("epi_name,epi", EPI_CASES, ids=[e[0] for e in EPI_CASES])
@pytest.mark.parametrize("M", [M_BELOW, M_ROWS], ids=["below_2_31", "above_2_31"])
def test_linear_f32_large_a_on_both_sides_of_the_route_switch(dev, M, epi_name, epi):
    """(M, 128, 3072): M * K just below 0x7fffffff takes the stream-K tail (32-bit element offsets into A), just above it the
    persistent whole-tile kernel — with or without the stream-K scratch, where the launch above the boundary has the same bits."""
    N, K = 128, LD
    want = F["STREAMK_TAIL"] if M == M_BELOW else F["PERSISTENT"]
    assert lib().gdr_linear_f32_form(M, N, K, STREAMK_BYTES) == want and lib().gdr_linear_f32_form(M, N, K, 0) == F["PERSISTENT"]
    op = _linear_operands(dev)
    A = op["A"][:M]
    W = _randn(N, K, 41, dev, scale=K ** -0.5)
    bias = _randn(1, N, 42, dev)[0] if epi != _ffi.EPI_NONE else None
    R = _randn(M, N, 43, dev) if epi != _ffi.EPI_NONE else None
    win = _windows(M, [b for b in (M32B, M31) if b + 128 <= M], dev)
    outs = []
    for ws in (op["ws"], None):
        C_ = R.clone() if R is not None else torch.full((M, N), float("nan"), device=dev)
        _f32_linear(A, K, W, C_, N, M, N, K, epi, bias, C_ if R is not None else None, N, ws)
        _no_fault("linear")
        _check_linear(C_, lambda r: A[r], W, bias, (lambda r: R[r]) if R is not None else None, M, win,
                      f"f32 {M} x {N} x {K} {epi_name} ws {'yes' if ws is not None else 'no'}")
        outs.append(C_)
    if M == M_ROWS:
        assert _same_bits(outs[0], outs[1]), "above the boundary the scratch must not change the kernel or the k order"


@pytest.mark.parametrize("K", [64, 320])
def test_linear_f32_large_c_and_residual_small_a(dev, K):
    """(700 001, 3072, K), BIAS_RESIDUAL with the residual aliasing C: C is 8.6 GB, A is small and DENSE (lda = K, 0.18 / 0.9 GB), so
    streamk_fits(M, lda, N, ldw) holds and the launcher takes the form gdr_linear_f32_form reports (asserted below):
      K = 64  — PERSISTENT with the scratch and without (two K-steps: the tail of 131 256 tiles is never worth a hand-off);
      K = 320 — STREAMK_TAIL with the scratch, PERSISTENT without: the stream-K epilogue addresses C and the residual past 2^31
                elements, and its result must have the bits of the whole-tile kernel.
    Dense, and ldc = ldr = 3072 + 64 with NaN in the pad columns.  The case owns its operands (the shared 8.6 GB A is dropped)."""
    M, N = M_ROWS, LD
    forms = (lib().gdr_linear_f32_form(M, N, K, STREAMK_BYTES), lib().gdr_linear_f32_form(M, N, K, 0))
    assert forms == ((F["PERSISTENT"], F["PERSISTENT"]) if K == 64 else (F["STREAMK_TAIL"], F["PERSISTENT"])), forms
    assert M * K < 0x7fffffff and N * K < 0x7fffffff <= M * N               # what streamk_fits looks at, and what it does not
    _drop("corpus", "linear")
    _assert_released("case 5")
    _need(dev, 30 << 30, "three [700 001, 3072] fp32 tensors and reference chunks")
    A = _randn(M, K, 50, dev)
    W = _randn(N, K, 51, dev, scale=K ** -0.5)
    bias = _randn(1, N, 52, dev)[0]
    R = _randn(M, N, 53, dev)
    scratch = torch.empty(STREAMK_BYTES, dtype=torch.uint8, device=dev)
    win = _windows(M, [M32B, M31], dev)
    first = None
    for ws in (scratch, None):
        C_ = R.clone()
        _f32_linear(A, K, W, C_, N, M, N, K, _ffi.EPI_BIAS_RESIDUAL, bias, C_, N, ws)
        _no_fault("linear")
        _check_linear(C_, lambda r: A[r], W, bias, lambda r: R[r], M, win, f"f32 {M} x {N} x {K} ws {'yes' if ws is not None else 'no'}")
        if first is None:
            first = C_
        else:
            assert _same_bits(first, C_), "the result depends on the scratch"
            del C_
    ld = N + 64
    for ws in (scratch, None):
        Cp = torch.full((M, ld), float("nan"), device=dev)
        for lo, hi in _chunks(M, 1 << 17):
            Cp[lo:hi, :N] = R[lo:hi]
        _f32_linear(A, K, W, Cp, ld, M, N, K, _ffi.EPI_BIAS_RESIDUAL, bias, Cp, ld, ws)
        _no_fault("linear, padded")
        assert bool(torch.isnan(Cp[win][:, N:]).all()), "a pad column of C was written"
        assert not bool(torch.isnan(Cp[win][:, :N]).any())
        assert all(torch.equal(Cp[lo:hi, :N], first[lo:hi]) for lo, hi in _chunks(M, 1 << 17)), "ldc = ldr = 3136 differs from the dense result"
        del Cp
    del first, R, A, scratch
    _drop()


@pytest.mark.parametrize("epi_name,epi", EPI_CASES, ids=[e[0] for e in EPI_CASES])
@pytest.mark.parametrize("N,K", [(128, LD), (LD, 64)], ids=["large_a", "large_c"])
def test_linear_bf16_large_a_and_large_c(dev, N, K, epi_name, epi):
    """gdr_linear_bf16 at (700 001, 128, 3072) — A in bf16 is 4.3 GB, byte 2^32 in row 699 050 — and at (700 001, 3072, 64).
    gdr_linear_bf16_tile_form reports 192 for the first (a 256-row tile: asserted as 192 or 256, whichever a retuned cost model
    picks) and 128 for the second (the 128-row tile; printed, the case does not depend on it)."""
    M = M_ROWS
    form = lib().gdr_linear_bf16_tile_form(M, N, K, epi)
    print(f"gdr_linear_bf16_tile_form({M}, {N}, {K}, {epi_name}) = {form}")
    if N == 128:
        assert form in (192, 256), f"the large-A shape must take the 256-row tile, not form {form}"
    op = _linear_operands(dev)
    A16 = torch.empty((M, K), dtype=torch.bfloat16, device=dev)
    for lo, hi in _chunks(M, 1 << 17):
        A16[lo:hi] = op["A"][lo:hi, :K].bfloat16()                               # torch's rounding
    assert K != LD or A16.numel() * 2 >= 2 ** 32
    W16 = _randn(N, K, 61, dev, scale=K ** -0.5).bfloat16()
    bias = _randn(1, N, 62, dev)[0] if epi != _ffi.EPI_NONE else None
    R = _randn(M, N, 63, dev) if epi != _ffi.EPI_NONE else None
    C_ = R.clone() if R is not None else torch.full((M, N), float("nan"), device=dev)
    _check(lib().gdr_linear_bf16(ptr(A16), K, ptr(W16), K, ptr(C_), N, M, N, K, epi, ptr(bias), ptr(C_ if R is not None else None), N, stream_ptr()),
           "gdr_linear_bf16")
    _no_fault("linear_bf16")
    bounds = [M31] if K == LD else []                                            # bf16 A: byte 2^32 = element 2^31
    if N == LD:
        bounds = [M32B, M31]                                                     # fp32 C / residual
    _check_linear(C_, lambda r: A16[r], W16, bias, (lambda r: R[r]) if R is not None else None, M, _windows(M, bounds, dev),
                  f"bf16 {M} x {N} x {K} {epi_name}")
    del C_, R, A16
    _drop()


@pytest.mark.parametrize("terms,bound", [(6, 3e-5), (2, 1.5e-5)])
def test_split_planes_and_split_linear_past_2_31_elements(dev, terms, bound):
    """gdr_split_f32_bf16x3 / gdr_split_f32_f16x2 on [700 001, 1536] (plane buffers of 3.2 G / 2.15 G elements), the whole output
    against torch's expressions (test_split_and_cast_write_their_rows_only), then gdr_linear_split_bf16 with N = 128 on them: the
    whole product against torch's fp32 at TOL and the windows against float64 within `bound` x mean |c|
    (test_linear_split_forms_and_leading_dimensions)."""
    M, N, K = M_ROWS, 128, 1536
    op = _linear_operands(dev)
    x = op["A"][:, :K].contiguous()
    w = _randn(N, K, 71, dev, scale=K ** -0.5)
    planes = 2 if terms == 2 else 3
    ld = lib().gdr_split_row_elems(K, terms)
    assert ld == planes * K and M * ld >= 2 ** 31
    a3 = ops.split_f16x2(x) if terms == 2 else ops.split_bf16x3(x)
    _no_fault("split")
    assert tuple(a3.shape) == (M, ld)
    for lo, hi in _chunks(M, 1 << 17):
        xc = x[lo:hi]
        if terms == 2:
            hi_ = xc.half()
            want = torch.cat([hi_, ((xc - hi_.float()) * 2048.0).half()], 1)
        else:
            hi_ = xc.bfloat16()
            mid = (xc - hi_.float()).bfloat16()
            want = torch.cat([hi_, mid, (xc - hi_.float() - mid.float()).bfloat16()], 1)
        assert torch.equal(a3[lo:hi], want), f"planes of rows [{lo}, {hi})"
    w3 = ops.split_f16x2(w) if terms == 2 else ops.split_bf16x3(w)
    out = ops.linear_split_bf16(a3, w3, K, terms=terms)
    _no_fault("linear_split")
    win = _windows(M, [2 ** 31 // ld], dev)                                      # 2-byte planes: element 2^31 = byte 2^32
    _check_linear(out, lambda r: x[r], w, None, None, M, win, f"split linear terms {terms}")
    ref = x[win].double() @ w.double().T
    worst, mean = float((out[win].double() - ref).abs().max()), float(ref.abs().mean())
    print(f"split linear terms {terms}: max |c - float64| on the windows = {worst:.3e} = {worst / mean:.3e} x mean |c| (bound {bound:.1e})")
    assert worst <= bound * mean
    del a3, out, x
    _drop()


# ================================================================================================ idx_offset at the top of int32
def test_sim_topk_ids_at_the_top_of_the_int32_range(dev):
    """ids are row + idx_offset in int32: N = 70 001 with idx_offset = 2^31 - 1 - N puts the last document at 2^31 - 2, the largest
    id the entry points admit.  Exact against the oracle for the fp32, bf16 and pre-filter forms, stream (B = 8) and tiled (B = 40)."""
    from conftest import order_insensitive_topk_match
    from oracle import retrieval_ref
    N, d, k = 70_001, 128, 20
    off = 2 ** 31 - 1 - N
    g = torch.Generator().manual_seed(9)
    D = torch.randn(N, d, generator=g)
    Q = torch.randn(B_MAX, d, generator=g)
    Q[3] = D[N - 1]                                                               # the last document is a rank-1 hit
    Dd, Qd = D.to(dev), Q.to(dev)
    P = ops.PrefilteredCorpus(Dd)
    for B in (8, B_MAX):
        for name, target, Qr, Dr in (("f32", Dd, Q, D), ("bf16", P.D16, Q.bfloat16().float(), D.bfloat16().float()), ("prefilter", P, Q, D)):
            v, i, st = ops.sim_topk(Qd[:B], target, k, idx_offset=off, return_status=True, exact_on_overflow=False)
            assert int(st.abs().sum()) == 0 and i.dtype == torch.int32
            i64 = i.cpu().numpy().astype(np.int64)
            assert i64.min() >= off and i64.max() == 2 ** 31 - 2 and i64[3, 0] == 2 ** 31 - 2, (name, B)
            rv, ri = retrieval_ref.sim_topk(Qr[:B], Dr, k)
            order_insensitive_topk_match(rv.numpy(), ri.numpy(), v.cpu().numpy(), i64 - off, TOL)
    # one more: refused, nothing written
    v = torch.zeros((8, k), device=dev)
    i = torch.zeros((8, k), dtype=torch.int32, device=dev)
    ws = torch.empty(lib().gdr_sim_topk_workspace_bytes(8, N, d, k, 0), dtype=torch.uint8, device=dev)
    rc = lib().gdr_sim_topk(ptr(Qd), 8, ptr(Dd), N, d, k, off + 1, ptr(v), ptr(i), None, 0, ptr(ws), ws.numel(), stream_ptr())
    torch.cuda.synchronize()
    assert rc == _ffi.GDR_EINVAL and b"idx_offset" in lib().gdr_last_error() and not bool(i.any())
