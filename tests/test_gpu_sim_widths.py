"""The similarity top-k at every kind of embedding width its contract admits (gdr_sim_topk, gdr_sim_topk_bf16, gdr_sim_topk_prefilter;
inputs and expected lists: tests/sim_widths.py, checked on the host by tests/test_sim_widths_host.py).  Six contraction paths have
width code of their own:

  fp32 tiled core, K-tail branch (gemm_nt_f32_kernel + sim epilogues, d % 32 != 0)   d = 4 8 28 36 60 100 132 1028 (32, 64: no tail)
  fp32 stream kernels, ring over d / 32 groups (B <= 32, d % 128 == 0, d <= 1024)    d = 128 256 .. 1024 (4 8 .. 32 groups)
  fp32 split-K sample kernel (sim_stream_sample_splitk_kernel)                       the sample pass of the same calls
  bf16 LDS-DMA core (launch_sim_bf16_glds, d % 64 == 0)                              d = 64 192 320 1088, and 256 .. 2048 at B > 32
  bf16 generic core + sim epilogues (gemm_nt_f32_kernel<.., true>, d % 64 != 0)      d = 8 24 40 72 136 1032
  bf16 stream kernels, ring over d / 64 groups (B <= 32, d % 256 == 0, d <= 2048)    d = 256 512 .. 2048

and the pre-filter adds sim_qprep_kernel and the fp32 rescoring of prefilter_tail_kernel (four 256-column pieces behind `col < d`):
d = 8 40 72 256 264 520 1016 1024.  The main oracle is EXACT: integer inputs, one expected list for all three entry points,
torch.equal on ids and values, exact_on_overflow=False and status == 0, so that the form under test — not the repair — answered.
Float inputs whose end pieces carry half of each row's norm are then held against float64, and the rerank's dot product runs at
d = 4, 36, 260 and 1028."""
import math

import numpy as np
import pytest
import torch

import sim_widths as sw
from conftest import order_insensitive_topk_match, ranked_lists_match
from gdr_amd import _ffi, ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.set_grad_enabled(False)
    return torch.device("cuda:0")


_DEV = {}


def _on_dev(d, dev):
    """(Q, D fp32, D bf16) of width d on the device; one width is resident at a time (the tests walk the widths in order)"""
    if d not in _DEV:
        _DEV.clear()
        Qn, Dn = sw.ints(d)
        D = torch.from_numpy(Dn).to(dev)
        _DEV[d] = (torch.from_numpy(Qn).to(dev), D, D.bfloat16())
    return _DEV[d]


def _run(Q, D, k, flags=0, idx_offset=0):
    """the call under test with the repair switched off: status must be 0"""
    v, i, st = ops.sim_topk(Q, D, k, idx_offset=idx_offset, return_status=True, exact_on_overflow=False, flags=flags)
    assert int(st.sum()) == 0, "a candidate list overflowed"
    return v.cpu(), i.cpu()


def _check(Q, D, d, N, k, B, flags=0, idx_offset=0, what=""):
    ev, ei = sw.expected(d, N, k)
    v, i = _run(Q[:B].contiguous(), D[:N], k, flags, idx_offset)
    case = (what, f"d={d} N={N} k={k} B={B} flags={flags}")
    assert torch.equal(i, ei[:B] + idx_offset), case + ("ids",)
    assert torch.equal(v, ev[:B]), case + ("values",)


# ---- 1. exact lists: dense fp32 and bf16 corpora ---------------------------------------------------------------------------------
@pytest.mark.parametrize("corpus,d", [(c, d) for c in ("fp32", "bf16") for d in sorted(sw.widths(c))], ids=lambda x: str(x))
def test_integer_scores_give_the_exact_list_at_every_width(dev, corpus, d):
    Q, D32, D16 = _on_dev(d, dev)
    D = D32 if corpus == "fp32" else D16
    if corpus == "bf16":
        assert torch.equal(D16.float(), D32)
    for N, k in sw.SHAPES:
        for B, no_stream in sw.batches(corpus, d):
            _check(Q, D, d, N, k, B, _ffi.SIM_NO_STREAM if no_stream else 0, what=corpus)
    if d == sw.EXTRA_WIDTH[corpus]:
        _check(Q, D, d, sw.N_BIG, sw.K_BIG, 7, idx_offset=1000, what=corpus + " idx_offset")
        for N, k in sw.SHAPES:
            _check(Q, D, d, N, k, 7, _ffi.SIM_EXHAUSTIVE, what=corpus + " exhaustive")
    if d in sw.DEEP_WIDTHS[corpus]:
        for k in (1, 100):
            for B, no_stream in sw.batches(corpus, d):
                if B in (7, 129):
                    _check(Q, D, d, sw.N_BIG, k, B, _ffi.SIM_NO_STREAM if no_stream else 0, what=corpus)


# ---- 2. exact lists: the pre-filter ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", sw.PREFILTER)
def test_prefilter_gives_the_exact_list_and_the_fp32_paths_bits(dev, d):
    """The bf16 pass takes the generic core at d = 8, 40, 72, 264, 520, 1016 and the LDS-DMA core / the stream kernels (B = 7) at 256,
    1024; the rescoring's `col < d` guard is false for SOME lanes of a 256-column piece wherever d % 256 != 0.
    dnorm_max: the squared norm is an exact integer here, ops.PrefilteredCorpus puts (1 + 1e-6) on its root on purpose (an upper
    bound is what the band needs), so the figure sits AT 1e-6: it is taken relative to the larger of the two, as math.isclose does."""
    Q, D32, _ = _on_dev(d, dev)
    P = ops.PrefilteredCorpus(D32)
    want = math.sqrt(float((sw.ints(d)[1].astype(np.int64) ** 2).sum(1).max()))
    print(f"d={d}: dnorm_max {P.dnorm_max!r}, float64 {want!r}, relative {abs(P.dnorm_max - want) / want:.3e}")
    assert P.dnorm_max >= want and math.isclose(P.dnorm_max, want, rel_tol=1e-6, abs_tol=0.0)
    for k in (sw.K_BIG, 100) if d in sw.PREFILTER_K100 else (sw.K_BIG,):
        ev, ei = sw.expected(d, sw.N_BIG, k)
        for B in sw.PREFILTER_B:
            q = Q[:B].contiguous()
            pv, pi = _run(q, P, k)
            assert torch.equal(pi, ei[:B]) and torch.equal(pv, ev[:B]), (d, k, B, "pre-filter against the expected list")
            fv, fi = _run(q, D32, k)
            assert torch.equal(pi, fi) and torch.equal(pv, fv), (d, k, B, "pre-filter against the fp32 path")


# ---- 3. float inputs against float64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", [(kind, d) for kind, ws in sw.FLOAT_WIDTHS.items() for d in ws], ids=lambda x: str(x))
def test_float_scores_against_float64(dev, kind, d):
    """Unit rows whose first and last 16-byte pieces carry half of the squared norm: a dropped or doubled end piece moves a score
    by tenths.  Tolerance from the inputs (sim_widths.float_tolerance).  The measured
    maximum error of each call is printed before the rule is applied.  Measured on the MI355X, the largest |value - float64 score
    of its id| over the calls of a case (its tolerance): fp32 36: 1.7e-7 (1e-4), 896: 6.6e-7 (1.07e-4), 1028: 5.7e-7 (1.23e-4);
    bf16 72: 5.5e-8 (1e-5), 1792: 2.2e-7 (2.15e-4), 2048: 2.6e-7 (2.45e-4); pre-filter 264: 7.5e-8 (1e-4), 1016: 7.5e-8 (1.22e-4)."""
    Qn, Dn = sw.floats(kind, d)
    Q64, D64, s = sw.float_reference(kind, d)
    tol, band = sw.float_tolerance(kind, d, Q64, D64)
    rv, ri = sw.float_topk(s, sw.FLOAT_K)
    Q, D = torch.from_numpy(Qn).to(dev), torch.from_numpy(Dn).to(dev)
    target = {"fp32": lambda: D, "bf16": lambda: D.bfloat16(), "prefilter": lambda: ops.PrefilteredCorpus(D)}[kind]()
    stream = kind != "prefilter" and sw.stream_eligible(kind, d)
    for B, flags in [(b, 0) for b in sw.FLOAT_B] + ([(min(sw.FLOAT_B), _ffi.SIM_NO_STREAM)] if stream else []):
        v, i = _run(Q[:B].contiguous(), target, sw.FLOAT_K, flags)
        v, i = v.numpy(), i.numpy().astype(np.int64)
        err = np.abs(v - np.take_along_axis(s[:B], i, 1)).max()
        print(f"{kind} d={d} B={B} flags={flags}: max |value - float64 score of its id| = {err:.3e}, tolerance {tol:.3e} (band {band:.3e})")
        order_insensitive_topk_match(rv[:B], ri[:B], v, i, tol)


# ---- 4. the rerank's dot product -------------------------------------------------------------------------------------------------
RERANK_TOL = 1e-4            # tests/test_gpu_rerank.py


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("d", sw.RERANK_WIDTHS)
def test_rerank_dot_product_at_other_widths(dev, d, bf16):
    """gdr_rerank_topk / gdr_rerank_topk_bf16 read a row in 16-byte (fp32) or 8-byte (bf16) pieces of four columns: one piece, nine,
    65 (one past a wave's 64 lanes) and 257.  Against oracle.retrieval_ref in float64, on the bf16-rounded rows for a bf16 corpus."""
    from oracle import retrieval_ref
    c = sw.rerank_case(d)
    B, R, k, alphas = c["B"], c["R"], c["k"], c["alphas"]
    D = torch.from_numpy(c["D"])
    Dd = D.to(dev).bfloat16() if bf16 else D.to(dev)
    Dref = (Dd.float().cpu() if bf16 else D).double()
    Q = torch.from_numpy(c["Q"])
    offs, ids, beam = (torch.from_numpy(c[x]).to(dev) for x in ("offsets", "ids", "beam"))
    for func in ("tanh", "sigmoid"):
        v, i = ops.rerank_topk(Q.to(dev), Dd, offs, ids, beam, alphas, k, func=func)
        v, i = v.cpu().numpy(), i.cpu().numpy()
        ref = retrieval_ref.rerank(Q.double(), Dref, c["mem"], [row.tolist() for row in c["sizes"]], c["beam"].tolist(), alphas, k, func=func)
        for b in range(B):
            for a in range(len(alphas)):
                rv, ri = ref[b][a]
                np.testing.assert_allclose(v[b, a], rv.numpy(), rtol=RERANK_TOL, atol=RERANK_TOL, err_msg=f"d={d} {func} b={b} a={a}")
                ranked_lists_match(ri.tolist(), rv.numpy(), i[b, a].tolist(), RERANK_TOL)
