"""k-means++ seeding of the hierarchical docid build on the MI355X (include/gdr_hip_kmeans_seed.h): one seeding step
and the whole seeding of a level against the numpy restatement (tests/kmeans_pp_ref.py) bit for bit — no margins —, the whole tree
against the fixture g16_kmeans_pp, the unchanged default, the degenerate cases, the memory contract and the refusals."""
import numpy as np
import pytest
import torch

import kmeans_pp_ref as pp
import kmeans_ref as kr
from abi_guard import guarded, guarded_input, poisoned_workspace
from conftest import golden
from gdr_amd import _ffi, kmeans, ops
from gdr_amd._ffi import lib, ptr, stream_ptr
from test_gpu_abi_memory import run_guarded, same_bits

pytestmark = pytest.mark.gpu
N = 1500


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.set_grad_enabled(False)
    return torch.device("cuda:0")


def _corpus(d, seed=3):
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((N, d)) * rng.uniform(0.25, 4.0, (N, 1))).astype(np.float32)
    X[10:30] = X[7]                                                   # duplicate rows: distance exactly 0 to one another
    return X


def _level(rng, k, one, outside=True):
    """(rows, offsets): one node of all N rows, or 12 nodes of sizes 1, k, k + 1, tile - 1, tile, tile + 1, about 5 tiles, ...; with
    `outside` the last row of the last node is an id outside the corpus (it reads as a zero row)."""
    tile = lib().gdr_kmeans_seed_tile()
    sizes = [N] if one else [1, k, k + 1, tile - 1, tile, tile + 1, 5 * tile + 3, 2, 40, 17, 64, 33]
    assert sum(sizes) <= N and tile == 128
    perm = rng.permutation(N)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    rows = np.concatenate([np.sort(perm[off[i]:off[i + 1]]) for i in range(len(sizes))]).astype(np.int32)
    if outside and not one:
        rows[-1] = N + 5
    return rows, off


def _step_case(d, k, one):
    """A mid-seeding state of the level: every node has its first member as the one chosen centre (d2, e from the restatement), node 1
    of the 12 is still before its first centre (d2 = +inf, a single candidate); candidates are members, with a -1, an id outside the
    corpus and duplicate rows among them."""
    rng = np.random.default_rng(100 * d + k)
    X = _corpus(d)
    rows, off = _level(rng, k, one)
    S, T = len(off) - 1, pp.n_trials(k)
    d2 = np.empty(len(rows), np.float32)
    e = np.zeros(S, np.int32)
    cand = np.empty((S, T), np.int32)
    for s in range(S):
        r = rows[off[s]:off[s + 1]]
        cand[s] = rng.choice(r[r < N], T)
        first = np.full(T, -1)
        first[0] = r[0]
        d2[off[s]:off[s + 1]] = pp.step_columns(X, r, first, np.full(len(r), np.inf, np.float32), 0)[0][:, 0]
        e[s] = pp.exponent(d2[off[s]:off[s + 1]].max())
    if one:
        cand[0, 0], cand[0, T - 1] = 12, -1                           # a duplicate row; no candidate
    else:
        d2[off[1]:off[2]], e[1], cand[1, 1:] = np.inf, 0, -1
        cand[3, 1], cand[6, 0], cand[4, T - 1] = -1, N + 5, 12
    return X, rows, off, cand, d2, e


@pytest.mark.parametrize("one", [True, False], ids=["1node", "12nodes"])
@pytest.mark.parametrize("k", [2, 8, 30, 64])
@pytest.mark.parametrize("d", [4, 32, 100, 768])
def test_one_seeding_step_equals_the_restatement_bit_for_bit(dev, d, k, one):
    X, rows, off, cand, d2, e = _step_case(d, k, one)
    S, T = cand.shape
    assert T == {2: 2, 8: 4, 30: 5, 64: 6}[k]
    t = lambda a: torch.from_numpy(a).to(dev)    # noqa: E731
    work = ops.kmeans_worklist(t(off), lib().gdr_kmeans_seed_tile())
    cd, pot, mx, st = ops.kmeans_seed_dist(t(X), t(rows), t(off), t(cand), t(d2), t(e), work=work)
    assert int(st.item()) == 0
    cd, pot, mx, work = cd.cpu().numpy(), pot.cpu().numpy(), mx.cpu().numpy(), work.cpu().numpy()
    want = np.concatenate([pp.step_columns(X, rows[off[s]:off[s + 1]], cand[s], d2[off[s]:off[s + 1]], e[s])[0] for s in range(S)])
    assert np.array_equal(cd.view(np.uint32), want.view(np.uint32)), f"{int((cd.view(np.uint32) != want.view(np.uint32)).sum())} distances differ"
    if one:                                                           # candidate 12 is one of the duplicates: exactly 0 for all 21 of them
        dup = np.isin(rows, np.r_[7, 10:30])
        assert dup.sum() == 21 and (want[dup, 0] == 0).all()
    node_pot = np.zeros((S, T), np.int64)
    for i, (s, p) in enumerate(work):                                 # per tile: the maxima; per node: the summed potentials
        tile = want[p:min(off[s + 1], p + 128)]
        assert np.array_equal(mx[i].view(np.uint32), tile.max(0).view(np.uint32)), f"maxima of tile {i}"
        node_pot[s] += pot[i]
    for s in range(S):
        assert np.array_equal(node_pot[s], pp.step_columns(X, rows[off[s]:off[s + 1]], cand[s], d2[off[s]:off[s + 1]], e[s])[1]), f"node {s}"


@pytest.mark.parametrize("d,k", [(100, 8), (32, 30), (768, 2)])
def test_full_seeding_of_a_level_equals_the_restatement(dev, d, k):
    """All k - 1 steps, 2 restarts, random data, no margins: the chosen doc ids are the restatement's."""
    X = _corpus(d, seed=11)
    rows, off = _level(np.random.default_rng(d + k), k, False, outside=False)
    D, R, O = torch.from_numpy(X).to(dev), torch.from_numpy(rows).to(dev), torch.from_numpy(off).to(dev)
    for r in range(2):
        got, st = kmeans.seed_level(D, R, O, k, seed=5, restart=r, level=3, init="k-means++")
        want = pp.seed_level(X, rows.astype(np.int64), off, k, 5, r, 3)
        assert int(st.item()) == 0 and np.array_equal(got.cpu().numpy(), want), f"restart {r}"
        hashed, _st = kmeans.seed_level(D, R, O, k, seed=5, restart=r, level=3)
        assert np.array_equal(hashed.cpu().numpy(), np.stack([kr.init_rows(rows[off[s]:off[s + 1]].astype(np.int64), k, 5, r, 3)
                                                              for s in range(len(off) - 1)]))
    # a node seeded alone gets the seeds it gets inside the level
    s = 6
    alone, _st = kmeans.seed_level(D, R[off[s]:off[s + 1]].contiguous(), torch.tensor([0, off[s + 1] - off[s]], dtype=torch.int32, device=dev),
                                   k, seed=5, restart=1, level=3, init="k-means++")
    assert np.array_equal(alone.cpu().numpy()[0], want[s])


def _same_tree(out, digits, lengths):
    assert np.array_equal(out.lengths, lengths), "id lengths differ"
    assert np.array_equal(out.digits, digits), "id digits differ"


def test_whole_tree_equals_the_fixture_and_the_default_is_unchanged(dev):
    g15, g16 = golden("g15_kmeans"), golden("g16_kmeans_pp")
    X, k, c, max_iter = g15["X"], int(g15["k"]), int(g15["c"]), int(g15["max_iter"])
    D = torch.from_numpy(X).to(dev)
    for n_init in (1, 4):
        out = kmeans.build_docids(D, k=k, c=c, seed=int(g16["seed"]), max_iter=max_iter, n_init=n_init, init="k-means++")
        _same_tree(out, g16[f"digits_n{n_init}"], g16[f"lengths_n{n_init}"])
        want = float(g16[f"tree_inertia_n{n_init}"])
        print(f"n_init={n_init}: device inertia {out.inertia:.9g}, restatement {want:.9g}")
        assert abs(out.inertia - want) <= 1e-4 * want and all(lv["init"] == "k-means++" for lv in out.levels)
        again = kmeans.build_docids(D, k=k, c=c, seed=int(g16["seed"]), max_iter=max_iter, n_init=n_init, init="k-means++")
        assert np.array_equal(out.digits, again.digits) and out.inertia == again.inertia
        assert np.array_equal(out.root_centroids.view(np.uint32), again.root_centroids.view(np.uint32))
    # init="hash", spelled out or left out, is g15's tree
    for n_init, key in ((1, "tree_inertia_n1"), (kmeans.DEFAULT_N_INIT, "tree_inertia_default")):
        stats = {}
        digits, _leaves = kr.build(X, k, c, int(g15["seed"]), max_iter, n_init, stats=stats)
        assert abs(stats["inertia"] - float(g15[key])) <= 1e-12 * float(g15[key])
        dg, ln = kr.pad_digits(digits)
        a = kmeans.build_docids(D, k=k, c=c, seed=int(g15["seed"]), max_iter=max_iter, n_init=n_init, init="hash")
        b = kmeans.build_docids(D, k=k, c=c, seed=int(g15["seed"]), max_iter=max_iter, n_init=n_init)
        _same_tree(a, dg, ln)
        _same_tree(b, dg, ln)
        assert a.inertia == b.inertia and all(lv["init"] == "hash" for lv in b.levels)
    # init_centroids still replaces the root's seeding
    C0 = torch.from_numpy(g15["C0"].astype(np.float32)).to(dev)
    a = kmeans.build_docids(D, k=k, c=X.shape[0], max_iter=5, init_centroids=C0, max_depth=2, init="k-means++")
    assert np.array_equal(a.digits[:, 0], g15["sk_labels_T5"]) and a.levels[0]["restarts"] == 1


def test_identical_rows_terminate(dev):
    X = np.tile(np.random.default_rng(1).standard_normal(16).astype(np.float32), (100, 1))
    out = kmeans.build_docids(torch.from_numpy(X).to(dev), k=4, c=6, n_init=2, max_depth=6, init="k-means++")
    digits, _leaves = pp.build(X, 4, 6, n_init=2)
    _same_tree(out, *kr.pad_digits(digits))
    assert len(set(out.docid_strings())) == 100 and np.diff(out.cluster_index.offsets).max() <= 6


def test_memory_contract_and_a_malformed_work_item(dev):
    """Guard bands around every output, inputs with live tails, bit-identical repeats; a non-NULL workspace is not touched (the step
    declares 0 bytes); a malformed work item writes nothing and sets status bit 2."""
    d, k = 100, 30
    X, rows, off, cand, d2, e = _step_case(d, k, False)
    S, T = cand.shape
    n = len(rows)
    work = ops.kmeans_worklist(torch.from_numpy(off).to(dev), lib().gdr_kmeans_seed_tile()).cpu()
    W = work.shape[0]
    Dd, dh = guarded_input(torch.from_numpy(X), tail=torch.full((64, d), 1e3))                 # a row id >= N reads as a ZERO row, not these
    Rd, rh = guarded_input(torch.from_numpy(rows), tail=torch.full((1024,), N - 1, dtype=torch.int32))
    Od, oh = guarded_input(torch.from_numpy(off), tail=torch.full((256,), n, dtype=torch.int32))
    Wd, wh = guarded_input(work, tail=torch.tensor([[S - 1, int(off[-2])]] * 256, dtype=torch.int32))   # well-formed items behind the list
    Cd, ch = guarded_input(torch.from_numpy(cand), tail=torch.zeros((64, T), dtype=torch.int32))
    Pd, ph = guarded_input(torch.from_numpy(d2), tail=torch.zeros(1024))
    Ed, eh = guarded_input(torch.from_numpy(e), tail=torch.full((256,), 40, dtype=torch.int32))
    need = lib().gdr_kmeans_seed_workspace_bytes(S, W, T)
    assert need == 0
    specs = {"cd": ((n, T), torch.float32), "pot": ((W, T), torch.int64), "mx": ((W, T), torch.float32), "status": ((1,), torch.int32)}

    def call(o, ws, nb, work_ptr=None, n_work=W):
        return lib().gdr_kmeans_seed_dist(ptr(Dd), N, d, ptr(Rd), n, ptr(Od), S, work_ptr or ptr(Wd), n_work, ptr(Cd), T, ptr(Pd), ptr(Ed),
                                          ptr(o["cd"]), ptr(o["pot"]), ptr(o["mx"]), ptr(o["status"]), ptr(ws), nb, stream_ptr())

    res = run_guarded(dev, specs, need, call, inputs=[dh, rh, oh, wh, ch, ph, eh], what="kmeans_seed_dist")
    assert int(res["status"][0]) == 0
    o = ops.kmeans_seed_dist(*(torch.from_numpy(a).to(dev) for a in (X, rows, off, cand, d2, e)))
    assert all(same_bits(res[nm], t) for nm, t in zip(("cd", "pot", "mx", "status"), o))
    # a workspace the caller hands over anyway stays as it is
    ws, wsh = poisoned_workspace(4096, 0x5A, dev)
    outs = {name: guarded(shape, dtype, dev) for name, (shape, dtype) in specs.items()}
    assert call({nm: v for nm, (v, _h) in outs.items()}, ws, 4096) == 0
    wsh.check("kmeans_seed_dist: workspace")
    assert bool((ws == 0x5A).all()) and same_bits(outs["cd"][0], res["cd"])
    # malformed items (no such node; a position outside the node): nothing but the status word is written
    bad = torch.tensor([[S, 0], [-1, 5], [2, int(off[4])], [0, -3]], dtype=torch.int32, device=dev)
    outs = {name: guarded(shape, dtype, dev) for name, (shape, dtype) in specs.items()}
    before = {nm: v.clone() for nm, (v, _h) in outs.items()}
    assert call({nm: v for nm, (v, _h) in outs.items()}, None, 0, work_ptr=ptr(bad), n_work=4) == 0
    torch.cuda.synchronize()
    for nm, (v, h) in outs.items():
        h.check(f"malformed work list: output {nm}")
        assert nm == "status" or same_bits(v, before[nm]), f"a malformed work item wrote {nm}"
    assert int(outs["status"][0][0]) == 2
    for h in (dh, rh, oh, wh, ch, ph, eh):
        h.unchanged("kmeans_seed_dist: an input")


def test_refusals(dev):
    X = torch.from_numpy(_corpus(32)[:300].copy()).to(dev)
    with pytest.raises(_ffi.GdrError, match="init='kmeans"):
        kmeans.build_docids(X, init="kmeans")
    with pytest.raises(_ffi.GdrError, match="init='random'"):
        kmeans.seed_level(X, torch.arange(300, dtype=torch.int32, device=dev), torch.tensor([0, 300], dtype=torch.int32, device=dev), 4,
                          init="random")
    with pytest.raises(_ffi.GdrError, match="bf16"):
        kmeans.build_docids(X.to(torch.bfloat16), init="k-means++")
    with pytest.raises(_ffi.GdrError, match="d=30"):
        kmeans.build_docids(X[:, :30].contiguous(), init="k-means++")
    for k in (1, 65):
        with pytest.raises(_ffi.GdrError, match=f"k={k}"):
            kmeans.build_docids(X, k=k, init="k-means++")
    rows, off = torch.arange(300, dtype=torch.int32, device=dev), torch.tensor([0, 300], dtype=torch.int32, device=dev)
    cand, d2, e = torch.zeros((1, 3), dtype=torch.int32, device=dev), torch.zeros(300, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(_ffi.GdrError, match="bf16"):
        ops.kmeans_seed_dist(X.to(torch.bfloat16), rows, off, cand, d2, e)
    with pytest.raises(_ffi.GdrError, match="d=30"):
        ops.kmeans_seed_dist(X[:, :30].contiguous(), rows, off, cand, d2, e)
    with pytest.raises(_ffi.GdrError, match="int32"):
        ops.kmeans_seed_dist(X, rows.long(), off, cand, d2, e)
    with pytest.raises(_ffi.GdrError, match=r"cand \(1, 7\)"):
        ops.kmeans_seed_dist(X, rows, off, torch.zeros((1, 7), dtype=torch.int32, device=dev), d2, e)
    with pytest.raises(_ffi.GdrError, match="d2 must be"):
        ops.kmeans_seed_dist(X, rows, off, cand, d2[:10], e)
