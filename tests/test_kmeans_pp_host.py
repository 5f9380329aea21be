"""k-means++ seeding of the docid build, host side (include/gdr_hip_kmeans_seed.h): the exported symbols and their
prototypes, the pre-launch refusals, the properties of the numpy restatement (tests/kmeans_pp_ref.py), the fixture g16_kmeans_pp
regenerated from the restatement, and the --init option of the tools.  Needs no GPU."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

import kmeans_pp_ref as pp
import kmeans_ref as kr
from conftest import GOLDEN, REPO, golden
from gdr_amd import _ffi

CTYPE = {"size_t": C.c_size_t, "int": C.c_int, "int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}
NAMES = {"gdr_kmeans_seed_tile", "gdr_kmeans_seed_workspace_bytes", "gdr_kmeans_seed_dist"}
HEADER = os.path.join(REPO, "include", "gdr_hip_kmeans_seed.h")


def _strip(text):
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_symbols_are_exported_and_the_header_prototypes_match_the_binding():
    protos = {m.group(2): (m.group(1), " ".join(m.group(3).split()))
              for m in re.finditer(r"\b(size_t|int)\s+(gdr_\w+)\s*\(([^;{}]*?)\)\s*;", _strip(open(HEADER).read()), flags=re.S)}
    assert set(protos) == set(_ffi.KMEANS_SEED_SIGNATURES) == NAMES
    assert not NAMES & (set(_ffi.SIGNATURES) | set(_ffi.PREFILTER_MASK_SIGNATURES) | set(_ffi.COMPACT_SIGNATURES))
    l = _ffi.lib()
    for name, (ret, params) in protos.items():
        fn = getattr(l, name)                                                  # AttributeError: the library does not export it
        res, args = _ffi.KMEANS_SEED_SIGNATURES[name]
        assert fn.restype is res is CTYPE[ret] and fn.argtypes == args
        want = [] if params == "void" else [C.c_void_p if "*" in p else CTYPE[p.split()[-2]] for p in params.split(",")]
        assert args == want, (name, params)
    assert l.gdr_abi_version() == 9 == _ffi.ABI_VERSION
    assert l.gdr_kmeans_seed_tile() == 128 and l.gdr_kmeans_seed_workspace_bytes(12, 40, 5) == 0


def test_the_main_header_includes_the_new_one_and_declares_none_of_it():
    import test_abi_memory_host as main_host
    main = open(os.path.join(REPO, "include", "gdr_hip.h")).read()
    assert '#include "gdr_hip_kmeans_seed.h"' in main, "gdr_hip.h must declare the whole ABI"
    code = re.sub(r"//[^\n]*", " ", _strip(main))
    for name in NAMES:
        assert name not in code, f"{name} appears in gdr_hip.h outside a comment"
    assert set(main_host._prototypes()) == set(_ffi.SIGNATURES) and len(_ffi.SIGNATURES) == 75     # gdr_hip.h's own set is what it was
    flat = " ".join(open(HEADER).read().replace("*", " ").split())
    for phrase in ("every subtraction, multiplication and addition rounded on its own", "s8[l] = p[l] + p[l + 8]", "denormals are kept",
                   "not of the tile, the node set or the launch", "reads as a zero row", "integer accumulation", "reads and writes nothing else"):
        assert phrase in flat, phrase


def test_every_refusal_comes_before_any_launch():
    l = _ffi.lib()
    p = C.c_void_p(1 << 20)
    n0 = l.gdr_launch_count()
    err = lambda: l.gdr_last_error()   # noqa: E731

    def call(D=p, N=1000, d=32, n_rows=500, S=3, n_work=6, T=4, out=p, status=p):
        return l.gdr_kmeans_seed_dist(D, N, d, p, n_rows, p, S, p, n_work, p, T, p, p, out, p, p, status, None, 0, None)

    for d in (0, 30, 4100):
        assert call(d=d) == _ffi.GDR_EINVAL and f"d={d}".encode() in err()
    for T in (0, 7, -1):
        assert call(T=T) == _ffi.GDR_EINVAL and f"n_trials={T}".encode() in err()
    assert call(N=0) == _ffi.GDR_EINVAL and b"N=0" in err()
    assert call(N=2 ** 31) == _ffi.GDR_EINVAL and b"N=" in err()
    assert call(n_rows=0) == _ffi.GDR_EINVAL and call(S=0) == _ffi.GDR_EINVAL and call(n_work=0) == _ffi.GDR_EINVAL and b"bad size" in err()
    assert call(D=None) == _ffi.GDR_EINVAL and call(out=None) == _ffi.GDR_EINVAL and call(status=None) == _ffi.GDR_EINVAL and b"null" in err()
    assert call(D=C.c_void_p((1 << 20) + 4)) == _ffi.GDR_EINVAL and b"aligned" in err()
    assert l.gdr_launch_count() == n0


# ---------------------------------------------------------------------------------------------------- the restatement
def _data(n=400, d=20, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, d)) * rng.uniform(0.5, 3.0, (n, 1))).astype(np.float32)


def test_trials_per_step():
    assert [pp.n_trials(k) for k in (2, 30, 64)] == [2, 5, 6]
    assert [pp.n_trials(k) for k in (3, 7, 8, 20, 21, 54, 55)] == [3, 3, 4, 4, 5, 5, 6]
    from gdr_amd import kmeans
    assert all(kmeans.n_trials(k) == pp.n_trials(k) for k in range(2, 65))


def test_the_distance_is_a_pinned_fp32_tree():
    X = _data(d=100)
    c = X[5]
    got = pp.dist2(X, c)
    assert got.dtype == np.float32 and got[5] == 0 and (got >= 0).all()
    # the tree spelled out for one row: 25 pieces over 16 partial sums, then 8, 4, 2, 1
    x = X[9]
    p = [np.float32(0)] * 16
    for piece in range(25):
        for j in range(4):
            t = np.float32(x[4 * piece + j] - c[4 * piece + j])
            p[piece % 16] = np.float32(p[piece % 16] + np.float32(t * t))
    for h in (8, 4, 2, 1):
        p = [np.float32(p[l] + p[l + h]) for l in range(h)]
    assert got[9].view(np.uint32) == p[0].view(np.uint32)
    assert abs(float(got[9]) - float(((x.astype(np.float64) - c) ** 2).sum())) <= 100 * 2.0 ** -23 * float(got[9])
    tiny = np.full((1, 4), 1e-22, np.float32)                                   # denormal squares are kept, not flushed
    assert pp.dist2(tiny, np.zeros(4, np.float32))[0] > 0


def test_weights_are_exact_integers_below_2_22():
    v = np.array([0.0, 1e-30, 0.75, 1.0, 1.9999999, np.inf], np.float32)
    assert pp.exponent(v[:5].max()) == 1 and pp.exponent(0.0) == 0 and pp.exponent(0.5) == 0 and pp.exponent(1.0) == 1
    w = pp.weights(v, 1)
    assert w.dtype == np.int64 and w.tolist() == [0, 0, 3 << 19, 1 << 21, (1 << 22) - 1, (1 << 22) - 1]
    assert pp.threshold((1 << 53) - 1, 10) == 9 and pp.threshold(0, 10) == 0 and pp.threshold(1 << 52, 7) == 3
    assert pp.threshold((1 << 53) - 1, (1 << 53) - 1) == (1 << 53) - 2          # the rounded product is kept below the potential


def test_first_centre_distinct_ids_and_the_small_node_rule():
    X = _data()
    ids = np.sort(np.random.default_rng(1).choice(400, 150, replace=False)).astype(np.int64)
    for k, r in ((8, 0), (30, 1), (64, 2)):
        trace = []
        got = pp.seed_node(X, ids, k, 7, r, 2, trace)
        keys = kr.mix(7, r, 2, ids)
        assert got[0] == ids[np.lexsort((ids, keys))[0]], "the first centre is the member with the smallest key"
        assert len(set(got.tolist())) == k and set(got.tolist()) <= set(ids.tolist())
        assert len(trace) == k - 1 and all(p > 0 and ch in cs and ps[cs.index(ch)] == min(ps) and len(cs) == pp.n_trials(k) for p, cs, ps, ch in trace)
    for m in (1, 5, 8):                                                         # m <= k: the hashed rule, untouched
        assert np.array_equal(pp.seed_node(X, ids[:m], 8, 7, 0, 1), kr.init_rows(ids[:m], 8, 7, 0, 1))


def test_zero_potential_falls_back_to_the_hashed_order():
    X = _data()
    X[50:90] = X[50]
    ids = np.arange(50, 90, dtype=np.int64)                                     # identical rows: the potential is 0 after the first centre
    got = pp.seed_node(X, ids, 8, 7, 0, 0)
    assert np.array_equal(got, kr.init_rows(ids, 8, 7, 0, 0))
    ids = np.concatenate([[3, 17], ids])                                        # three distinct rows: two greedy steps, then the hashed order
    trace = []
    got = pp.seed_node(X, ids, 8, 3, 1, 0, trace)
    hashed = kr.init_rows(ids, 8, 3, 1, 0)
    assert [p > 0 for p, _c, _p, _h in trace] == [True, True] + [False] * 5
    assert len({X[i].tobytes() for i in got[:3]}) == 3 and np.array_equal(got[3:], hashed[3:]) and got[0] == hashed[0]


def test_a_node_alone_and_inside_a_level_gets_the_same_seeds():
    X = _data()
    rng = np.random.default_rng(4)
    perm = rng.permutation(400)
    off = np.array([0, 120, 129, 300, 400])
    rows = np.concatenate([np.sort(perm[off[i]:off[i + 1]]) for i in range(4)]).astype(np.int64)
    level = pp.seed_level(X, rows, off, 8, 7, 1, 2)
    assert level.shape == (4, 8)
    for s in range(4):
        assert np.array_equal(level[s], pp.seed_node(X, rows[off[s]:off[s + 1]], 8, 7, 1, 2))
        other = np.concatenate([rows[off[s]:off[s + 1]], rows[off[s - 1]:off[s]] if s else rows[off[1]:off[2]]])
        o2 = np.array([0, off[s + 1] - off[s], len(other)])
        assert np.array_equal(pp.seed_level(X, other, o2, 8, 7, 1, 2)[0], level[s])
    # the draws depend on (seed, restart, level, the node's smallest id, step, trial) and on nothing else
    assert pp.draw(7, 1, 2, 5, 3, 0) == pp.draw(7, 1, 2, 5, 3, 0) < 1 << 53
    assert len({pp.draw(7, 1, 2, 5, 3, 0), pp.draw(8, 1, 2, 5, 3, 0), pp.draw(7, 0, 2, 5, 3, 0), pp.draw(7, 1, 3, 5, 3, 0), pp.draw(7, 1, 2, 6, 3, 0),
                pp.draw(7, 1, 2, 5, 4, 0), pp.draw(7, 1, 2, 5, 3, 1)}) == 7


# ---------------------------------------------------------------------------------------------------- the fixture
def test_the_fixture_regenerates_bit_for_bit_from_the_restatement():
    recipe = _load(os.path.join(GOLDEN, "make_golden_kmeans_pp.py"), "make_golden_kmeans_pp")
    g15, g16 = golden("g15_kmeans"), golden("g16_kmeans_pp")
    assert "X" not in g16.files and os.path.getsize(os.path.join(GOLDEN, "g16_kmeans_pp.npz")) < 64 << 10, "no second corpus is stored"
    again = recipe.restated(g15, seed=int(g16["seed"]))
    assert set(again) | {"pooled_inertia_ratio"} == set(g16.files)
    for name, v in again.items():
        a, b = np.asarray(v), g16[name]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name
    bound = float(g15["gap_bound"])
    assert float(g16["min_gap_n1"]) >= bound and float(g16["min_gap_n4"]) >= bound and float(g16["restart_lead_n4"]) >= recipe.LEAD
    assert g16["q_n_inits"].tolist() == [1, 2, 4] and g16["pooled_inertia_ratio"].shape == (3,)
    # the chosen ids of the trace are the seeds seed_node returns, and the stored trees differ from the hashed ones
    node, chosen = g16["seed_node_n4"], g16["seed_chosen_n4"].reshape(-1, int(g15["k"]) - 1)
    assert len(node) == len(chosen) and node[0].tolist() == [0, 0, 0]
    root = pp.seed_node(g15["X"], np.arange(g15["X"].shape[0]), int(g15["k"]), int(g16["seed"]), 0, 0)
    assert np.array_equal(root[1:], chosen[0])


@pytest.mark.parametrize("tool", ["build_index.py", "bench_kmeans.py"])
def test_the_tools_take_init(tool):
    text = open(os.path.join(REPO, "tools", tool)).read()
    assert re.search(r'add_argument\("--init",[^\n]*choices=kmeans\.INITS', text), tool
    if tool == "build_index.py":
        mod = _load(os.path.join(REPO, "tools", tool), "build_index_tool")
        ap = mod.parser()
        assert ap.parse_args(["--embeddings", "x.npy", "--out", "c.npz"]).init == "hash"
        assert ap.parse_args(["--embeddings", "x.npy", "--out", "c.npz", "--init", "k-means++"]).init == "k-means++"
        with pytest.raises(SystemExit):
            ap.parse_args(["--embeddings", "x.npy", "--out", "c.npz", "--init", "random"])
