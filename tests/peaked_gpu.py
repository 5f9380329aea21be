"""What the GPU comparisons of the peaked cases share (test_gpu_peaked.py, test_gpu_peaked_long.py): the printed comparisons of the two
bound rules and the generate() comparison.  No test lives here."""
import numpy as np
import pytest
import torch

import peaked as P
from oracle.parity_rules import beam_cut_explains_absence, hypothesis_lists_match

FP32_SETTINGS = [pytest.param(P.MODERATE, id="moderate"), pytest.param(P.STRONG, id="strong")]


def close(got, want, bound, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    print(f"{what}: max |gpu - float64 oracle| {np.abs(got - want).max():.2e} (bound {bound:.1e})")
    np.testing.assert_allclose(got, want, rtol=bound, atol=bound, err_msg=what)


def noise_close(got, want, table, what):
    d = np.abs(np.asarray(got, np.float64) - want)
    print(f"{what}: |gpu - bf16 emulation with float64 sums| max {d.max():.3e} mean {d.mean():.3e} "
          f"(bounds {4 * table['noise'][0]:.1e} / {4 * table['noise'][1]:.1e})")
    assert d.max() <= 4 * table["noise"][0] and d.mean() <= 4 * table["noise"][1], what


def statistics_close(got, want, table, what):
    """The bf16 rule where 4 x the recorded noise maximum exceeds the 3e-2 cap (bert-bf16, peaked.py): max and mean within 4 x the
    noise's, the 99th percentile within 4 x the noise's (which meets the cap), and no larger a share of elements over 3e-2 than the
    noise has over 3e-2 / 4."""
    noise_close(got, want, table, what)
    d = np.abs(np.asarray(got, np.float64) - want)
    print(f"{what}: 99th percentile {np.quantile(d, 0.99):.3e} (bound {4 * table['p99']:.1e}), share of elements over 3e-2 "
          f"{(d > 3e-2).mean():.2e} (bound {table['over']:.1e})")
    assert np.quantile(d, 0.99) <= 4 * table["p99"] and (d > 3e-2).mean() <= table["over"], what


def pooled_close(got, want, table, what):
    """A bf16 case's pooled rows: within 4 x the recorded noise maximum."""
    d = np.abs(np.asarray(got, np.float64) - want).max()
    print(f"{what}: max |gpu - bf16 emulation with float64 sums| {d:.3e} (bound {4 * table['noise'][0]:.1e})")
    assert d <= 4 * table["noise"][0], what


def to_dev(a, dev):
    return torch.from_numpy(a).to(dev)


def tower(bc, sd, dev, **kw):
    from gdr_amd.modeling import EncoderModel
    return EncoderModel.from_state_dict(bc, sd, dev, **kw)


def generate_vs_oracle(dev, name, st, what, **model_kw):
    from gdr_amd.modeling import GDRModel
    cfg, sd, ids, mask, R = P.generate_case(name, st)
    B = ids.shape[0]
    bound = P.fp32_bound(P.generate_row(name)["g"][st.name])
    ref, ref_sc, trace, ptrace = P.generate_oracle(name, st, True)
    (dec, sc), _ = GDRModel(cfg, sd, dev, **model_kw).generate(to_dev(ids, dev), attention_mask=to_dev(mask, dev),
                                                               max_length=cfg.max_output_length, num_beams=R, length_penalty=0.8,
                                                               num_return_sequences=R, output_scores=True)
    sc = np.array(sc, np.float64).reshape(B, R)
    close(sc, ref_sc, bound, f"{what} {st.name} beam scores ({B} x {R})")
    got = P.hypothesis_lists(dec.cpu().numpy(), B, R)
    moved = foreign = 0
    for b in range(B):
        def explain(hyp, b=b):         # a hypothesis the oracle's list lacks must have fallen at a cut of ITS search by a tie
            return beam_cut_explains_absence(trace, ptrace, b, R, cfg.decode_vocab_size, list(hyp), bound, final_cut=ref_sc[b, -1])
        m, f, _ = hypothesis_lists_match(ref[b], ref_sc[b], got[b], bound, explain_foreign=explain)
        moved, foreign = moved + m, foreign + f
    print(f"{what} {st.name}: of {B * R} hypotheses {moved} moved inside a tie group, {foreign} crossed a cut by a tie")
