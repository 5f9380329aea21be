#!/usr/bin/env python3
"""Generate tests/golden/g15_kmeans.npz by running the REFERENCE's Data_process/NQ_dataset/kmeans/kmeans.py itself (runpy, in a
temporary directory that holds the ../bert/*.tsv it reads; none of its text is copied) on a small full-mantissa fixture, with
sklearn's fit_predict wrapped to record every call's row set and labels.

Build-container only (needs the reference tree, sklearn and pandas), like make_golden_expand.py: only the arrays written here
(the fixture, the reference's outputs, sklearn's Lloyd results and the recorded margins) are committed.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_kmeans.py [path to the reference's kmeans.py]

The fixture seed is searched: the first one for which every margin below holds is taken, and the margins are stored.
  * (b) Lloyd from C0 (T = 50 covers T = 1, 2, 5): in every round every row's float64 gap between the best and the second-best
    score is >= 4 * (2d + 8) * 2^-24 * max|x|^2, and no cluster empties.
  * (c) the float64 build (tests/kmeans_ref.py) at n_init = 1 and at the default: the same gap condition over every (node,
    restart, round, row), and wherever restarts compete for a node the best inertia is below every other one by >= 1e-4
    relative (the fp32 rounding of a sum of <= 1,000 terms is far below that), so the chosen restart cannot flip.
  * quality: for every split the reference made, the restatement on the same rows; sum(our inertia) / sum(reference inertia)
    per n_init in {1, 2, 4, 8, 16}, pooled over the first 8 fixtures that satisfy the n_init-independent conditions (and stored
    for the committed one too).  The default n_init is the smallest with a pooled ratio <= 1.05.
"""
import contextlib
import io
import os
import pickle
import runpy
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

import kmeans_ref as kr    # noqa: E402

N, D_MODEL, K, C, SEED, MAX_ITER = 1000, 32, 8, 40, 7, 300
N_INITS = (1, 2, 4, 8, 16)
T_LIST = (1, 2, 5, 50)


def reference_script():
    """The reference's kmeans.py beside the GDR_model tree make_golden.py imports."""
    sys.path.insert(0, HERE)
    import make_golden
    return os.path.join(os.path.dirname(make_golden.REF), "Data_process", "NQ_dataset", "kmeans", "kmeans.py")


def make_fixture(seed):
    """Two-level mixture, full-mantissa fp32: 7 top directions x 6 sub-directions + noise, and two far rows (singleton leaves)."""
    rng = np.random.default_rng(seed)
    top = rng.standard_normal((7, D_MODEL)) * 1.0
    sub = rng.standard_normal((7, 6, D_MODEL)) * 0.55
    a, b = rng.integers(0, 7, N), rng.integers(0, 6, N)
    X = top[a] + sub[a, b] + 0.25 * rng.standard_normal((N, D_MODEL))
    far = rng.choice(N, 2, replace=False)
    X[far] = 1.5 * rng.standard_normal((2, D_MODEL))
    return (X / np.sqrt(D_MODEL)).astype(np.float32)


def gap_bound(X):
    return 4.0 * (2 * X.shape[1] + 8) * 2.0 ** -24 * float((X.astype(np.float64) ** 2).sum(1).max())


def check_lloyd_margin(X, C0):
    """min gap over every round of Lloyd from C0 (float64); None if a cluster empties."""
    gaps, emptied = [], []

    def on_round(t, gap, lab):
        gaps.append(gap.min())
        emptied.append(len(np.unique(lab)) < C0.shape[0])

    kr.lloyd(X, C0, 50, on_round)
    return None if any(emptied) else float(min(gaps))


def check_build_margin(X, n_init):
    """(min gap, min relative inertia lead of the winning restart) of the float64 build, plus the build."""
    gaps, inert = [], {}
    stats = {}
    digits, leaves = kr.build(X, K, C, SEED, MAX_ITER, n_init,
                              on_round=lambda path, r, t, gap, lab: gaps.append(gap.min()),
                              on_restart=lambda path, r, i: inert.setdefault(path, []).append(i), stats=stats)
    lead = np.inf
    for v in inert.values():
        if len(v) > 1:
            s = np.sort(v)
            lead = min(lead, (s[1] - s[0]) / s[0])
    return float(min(gaps)), float(lead), digits, leaves, stats["inertia"]


def run_reference(X, script):
    """Runs the reference script on X -> (id mapping list, recorded [(rows, labels)] in call order)."""
    import sklearn.cluster as sc
    row_of = {X[i].astype(np.float64).tobytes(): i for i in range(X.shape[0])}
    assert len(row_of) == X.shape[0], "duplicate fixture rows"
    calls = []

    def wrap(cls):
        orig = cls.fit_predict

        def fit_predict(self, data, *a, **kw):
            lab = orig(self, data, *a, **kw)
            rows = np.array([row_of[np.ascontiguousarray(r, np.float64).tobytes()] for r in data], np.int64)
            calls.append((rows, np.asarray(lab, np.int64).copy()))
            return lab
        cls.fit_predict = fit_predict
        return orig

    o1, o2 = wrap(sc.KMeans), wrap(sc.MiniBatchKMeans)
    cwd, argv = os.getcwd(), sys.argv
    try:
        with tempfile.TemporaryDirectory() as tmp:
            os.makedirs(os.path.join(tmp, "bert"))
            os.makedirs(os.path.join(tmp, "kmeans"))
            with open(os.path.join(tmp, "bert", "NQ_doc_content_embedding_bert_512.tsv"), "w") as f:
                for i in range(X.shape[0]):
                    f.write("\t".join([str(i), "u", "t", "b", "a", "0", "en", "|".join(repr(float(v)) for v in X[i])]) + "\n")
            os.chdir(os.path.join(tmp, "kmeans"))
            sys.argv = ["kmeans.py", "--v_dim", str(D_MODEL), "--k", str(K), "--c", str(C), "--seed", str(SEED)]
            with contextlib.redirect_stdout(io.StringIO()):
                runpy.run_path(script, run_name="__main__")
            with open(f"IDMapping_NQ_bert_512_k{K}_c{C}_seed_{SEED}.pkl", "rb") as f:
                mapping = pickle.load(f)
    finally:
        os.chdir(cwd)
        sys.argv = argv
        sc.KMeans.fit_predict, sc.MiniBatchKMeans.fit_predict = o1, o2
    return [[int(x) for x in mapping[i]] for i in range(X.shape[0])], calls


N_CALIBRATE = 8


def quality(X, calls):
    """(our inertia per n_init, the reference's inertia, depth of every recorded split) on the reference's own splits."""
    X64 = X.astype(np.float64)
    ref_inertia = 0.0
    for rows, lab in calls:
        Xn = X64[rows]
        cent = np.stack([Xn[lab == j].mean(0) if (lab == j).any() else np.zeros(D_MODEL) for j in range(K)])
        ref_inertia += float(((Xn - cent[lab]) ** 2).sum())
    assert np.array_equal(np.sort(calls[0][0]), np.arange(N))
    # depth of a recorded split: how many recorded ancestors contain its rows (the calls come in depth-first order)
    sets = [set(r.tolist()) for r, _ in calls]
    depth_of = [sum(1 for j in range(i) if s < sets[j]) for i, s in enumerate(sets)]
    ours = [sum(kr.split_node(X, np.sort(rows), K, SEED, depth_of[i], MAX_ITER, n_init)[1] for i, (rows, _l) in enumerate(calls))
            for n_init in N_INITS]
    return np.array(ours), ref_inertia, depth_of


def main():
    script = sys.argv[1] if len(sys.argv) > 1 else reference_script()
    from sklearn.cluster import KMeans
    # Phase 1: the first N_CALIBRATE fixtures that satisfy the n_init-independent conditions decide the default n_init from their
    # pooled inertia (choosing it on the one committed fixture would let the margin search, which a single restart passes most
    # easily, pick the default).  Phase 2: the first such fixture that also satisfies the margins at that default is committed.
    cands, default, chosen = [], None, None
    for fseed in range(15000, 60000):
        X = make_fixture(fseed)
        X64 = X.astype(np.float64)
        bound = gap_bound(X)
        C0 = X64[kr.init_rows(np.arange(N, dtype=np.int64), K, SEED, 0, 0)]
        g_b = check_lloyd_margin(X64, C0)
        if g_b is None or g_b < bound:
            continue
        g1 = check_build_margin(X, 1)[0]
        if g1 < bound:
            continue
        if default is None:
            ref_ids, calls = run_reference(X, script)
            if not any((np.bincount(lab, minlength=K) == 1).any() for _r, lab in calls):
                continue
            ours, ref_inertia, depth_of = quality(X, calls)
            cands.append((fseed, ours, ref_inertia))
            print("calibration fixture", fseed, dict(zip(N_INITS, np.round(ours / ref_inertia, 4))), flush=True)
            if len(cands) < N_CALIBRATE:
                continue
            pooled = sum(o for _s, o, _r in cands) / sum(r for _s, _o, r in cands)
            print("pooled inertia ratio ours / reference per n_init", dict(zip(N_INITS, np.round(pooled, 4))), flush=True)
            ok = [n for n, r in zip(N_INITS, pooled) if r <= 1.05]
            assert ok, f"no n_init <= 16 reaches 1.05 x the reference's inertia: {pooled} — seeding is the real next step"
            default = ok[0]
            continue
        gd, lead, digits, leaves, tree_inertia = check_build_margin(X, default)
        if gd < bound or (default > 1 and lead < 1e-4):
            continue
        ref_ids, calls = run_reference(X, script)
        if not any((np.bincount(lab, minlength=K) == 1).any() for _r, lab in calls):
            continue
        ours, ref_inertia, depth_of = quality(X, calls)
        ratios = ours / ref_inertia
        chosen = fseed
        break
    if chosen is None:
        raise SystemExit("no fixture seed satisfies the margins")

    # (a) the id rules: the restatement fed the reference's recorded labels reproduces the reference's mapping
    by_rows = {np.sort(r).tobytes(): (r, lab) for r, lab in calls}

    def recorded(ids, level, path):
        r, lab = by_rows[np.asarray(ids, np.int64).tobytes()]
        out = np.empty(len(ids), np.int64)
        out[np.searchsorted(ids, r)] = lab
        return out

    got, _leaves = kr.assemble_ids(N, K, C, recorded)
    assert got == ref_ids, "id assembly of the restatement != the reference's id mapping"

    # (b) sklearn's Lloyd from C0
    sk = {}
    for T in T_LIST:
        m = KMeans(n_clusters=K, init=C0, n_init=1, algorithm="lloyd", tol=0, max_iter=T).fit(X64)
        lab, cen, inertia, _r = kr.lloyd(X64, C0, T)
        assert np.array_equal(lab, m.labels_), f"restated Lloyd labels != sklearn at T={T}"
        assert np.abs(cen - m.cluster_centers_).max() < 1e-12
        sk[f"sk_labels_T{T}"] = m.labels_.astype(np.int32)
        sk[f"sk_centers_T{T}"] = m.cluster_centers_.astype(np.float64)
        sk[f"sk_inertia_T{T}"] = np.float64(m.inertia_)

    g1, _lead1, _d1, _lv1, inertia1 = check_build_margin(X, 1)
    rd, rl = kr.pad_digits(ref_ids)
    path = os.path.join(HERE, "g15_kmeans.npz")
    np.savez_compressed(
        path, X=X, k=np.int64(K), c=np.int64(C), seed=np.int64(SEED), max_iter=np.int64(MAX_ITER), fixture_seed=np.int64(fseed),
        ref_digits=rd, ref_lengths=rl,
        call_offsets=np.concatenate([[0], np.cumsum([len(r) for r, _ in calls])]).astype(np.int32),
        call_rows=np.concatenate([r for r, _ in calls]).astype(np.int32),
        call_labels=np.concatenate([lab for _, lab in calls]).astype(np.int32),
        call_depth=np.array(depth_of, np.int32), ref_inertia=np.float64(ref_inertia),
        C0=C0, T_list=np.array(T_LIST, np.int32), gap_bound=np.float64(bound), lloyd_min_gap=np.float64(g_b),
        n_inits=np.array(N_INITS, np.int32), inertia_ratio=np.array(ratios, np.float64), default_n_init=np.int64(default),
        pooled_inertia_ratio=np.array(pooled, np.float64), calibration_seeds=np.array([s_ for s_, _o, _r in cands], np.int64),
        build_min_gap_n1=np.float64(g1), build_min_gap_default=np.float64(gd), restart_lead_default=np.float64(lead),
        tree_inertia_n1=np.float64(inertia1), tree_inertia_default=np.float64(tree_inertia), **sk)
    print(path, os.path.getsize(path), "bytes; reference splits:", len(calls), "default n_init:", default,
          "gaps / bound:", g_b / bound, g1 / bound, gd / bound, "lead:", lead)


if __name__ == "__main__":
    main()
