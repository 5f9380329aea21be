"""The two-chain form of the pooled-only fp32 ragged encoder forward (csrc/encoder.hip, GDR_ENC_CHAINS=2: the batch's two halves
run as two independent packed forwards, one on the caller's stream and one on a side stream, every persistent / stream-K linear
capped at 256 workgroups) must give the SAME BITS as the one-chain form: sequences do not interact, GEMM rows are independent
and every whole-K kernel form sums in the same order.  The knob is read once per process, so each value runs in its own child
process (the pattern of test_gpu_streamk.py) and digests of `pooled` are compared; one child runs all cases.
t5-base widths (eligibility is in 128 x 128 tiles of the real widths), 2 layers, L = 40:
  B = 200   the smallest even batch whose halves both pack (100 x 40 rows: 32 row panels x 6 = 192 tiles)
  B = 201   uneven halves (100 + 101)
  B = 198   a half (99 x 40 rows: 31 panels x 6 = 186 tiles) falls below the packed form: one chain, by the launch count
  B = 256   the bench's length distribution (uniform 8..40)
  B = 200   first half at full length, second half at lengths 1..8 (very uneven chains)
  B = 200   a mask with a hole and an all-zero mask in each half
plus: a guarded, pre-poisoned workspace of exactly gdr_t5_encoder_ragged_workspace_bytes; a call with out_hidden (one chain);
the launch profiler around one forward (the linear class's time is the union of its launches' intervals: never more than the
wall time between two fences); one graph capture and replay."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import ctypes as C, hashlib, json, os, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from gdr_amd import ops, synth
from gdr_amd.ops import lib, ptr
from gdr_amd.config import GDRConfig
from abi_guard import poisoned_workspace
torch.set_grad_enabled(False)
dev = torch.device("cuda:0")
cfg = GDRConfig.base()
cfg.num_layers = 2
L = 40
sd = synth.make_state_dict(cfg, seed=77, with_decoder=False)
enc = ops.T5EncoderHandle(cfg, sd, dev)
dg = lambda t: hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()

def tokens(name):
    if name == "b200": return synth.make_tokens(200, L=L, seed=21, min_len=8)
    if name == "b201": return synth.make_tokens(201, L=L, seed=22, min_len=8)
    if name == "b198": return synth.make_tokens(198, L=L, seed=23, min_len=8)
    if name == "b256_bench": return synth.make_tokens(256, L=L, seed=24, min_len=8)
    ids, mask = synth.make_tokens(200, L=L, seed=25, min_len=L)           # every row at full length
    if name == "b200_uneven":
        lens = np.random.Generator(np.random.PCG64(26)).integers(1, 9, size=100)
        mask[100:] = (np.arange(L)[None, :] < lens[:, None]).astype(np.int64)
        ids[100:] *= mask[100:]
    if name == "b200_holes":
        for half in (0, 100):
            mask[half + 7, 5] = 0                                          # a hole: the row keeps all L positions and its mask
            mask[half + 31, :] = 0                                         # an empty mask row
    return ids, mask

out = {"digest": {}, "launches": {}}
for name in ["b200", "b201", "b198", "b256_bench", "b200_uneven", "b200_holes"]:
    ids, mask = tokens(name)
    it, mt = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)
    n0 = lib().gdr_launch_count()
    _, p = enc.forward(it, mt, want_hidden=False, ragged=True, live_rows_hint=int(mask.sum()))
    out["launches"][name] = lib().gdr_launch_count() - n0
    torch.cuda.synchronize()
    assert lib().gdr_device_fault_pending() == 0, lib().gdr_last_error()
    out["digest"][name] = dg(p)
    if name == "b201":                                                     # no row hint: the grids are sized for B * L
        _, p2 = enc.forward(it, mt, want_hidden=False, ragged=True)
        torch.cuda.synchronize()
        out["digest"]["b201_nohint"] = dg(p2)

# ---- out_hidden set: out of the two-chain form's scope
ids, mask = tokens("b200")
it, mt = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)
n0 = lib().gdr_launch_count()
h, p = enc.forward(it, mt, ragged=True, live_rows_hint=int(mask.sum()))
out["launches"]["b200_hidden"] = lib().gdr_launch_count() - n0
torch.cuda.synchronize()
out["digest"]["b200_hidden_pooled"] = dg(p)

# ---- a workspace of exactly the stated size between guard bands, poisoned with two fills, on a non-default stream
need = lib().gdr_t5_encoder_ragged_workspace_bytes(C.byref(enc.dims), 200, L)
stream = torch.cuda.Stream(device=dev)
for fill in (0x00, 0xFF):
    ws, wh = poisoned_workspace(need, fill, dev)
    pooled = torch.empty((200, cfg.d_model), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        rc = lib().gdr_t5_encoder_forward_ragged(C.byref(enc.struct), ptr(it), ptr(mt), 200, L, None, ptr(pooled), int(mask.sum()),
                                                 ptr(ws), need, ops.stream_ptr())
    assert rc == 0, lib().gdr_last_error()
    stream.synchronize()                                                   # the call is ordered on the caller's stream alone
    out["digest"][f"b200_guard_{fill:02x}"] = dg(pooled)
    wh.check("ragged workspace")
    del ws, wh
ws, wh = poisoned_workspace(need, 0, dev)
rc = lib().gdr_t5_encoder_forward_ragged(C.byref(enc.struct), ptr(it), ptr(mt), 200, L, None, ptr(pooled), -1, ptr(ws), need - 1,
                                         ops.stream_ptr())
out["one_byte_short_rc"] = rc
del ws, wh

# ---- the launch profiler around one forward: union of the linear launches' intervals against the wall time between two fences
enc.forward(it, mt, want_hidden=False, ragged=True, live_rows_hint=int(mask.sum()))
torch.cuda.synchronize()
assert lib().gdr_prof_enable(256) == 0
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
enc.forward(it, mt, want_hidden=False, ragged=True, live_rows_hint=int(mask.sum()))
e1.record()
torch.cuda.synchronize()
n_l, ms_l, w_l = (C.c_int64 * 8)(), (C.c_double * 8)(), (C.c_double * 8)()
assert lib().gdr_prof_collect(n_l, ms_l, w_l) == 0
out["prof"] = {"linear_launches": int(n_l[0]), "linear_ms": float(ms_l[0]), "wall_ms": float(e0.elapsed_time(e1))}

# ---- one capture of a pooled-only call, replayed
pooled_g = torch.empty((200, cfg.d_model), dtype=torch.float32, device=dev)
ws_g = torch.empty(need, dtype=torch.uint8, device=dev)
torch.cuda.synchronize()
graph = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph):
    rc = lib().gdr_t5_encoder_forward_ragged(C.byref(enc.struct), ptr(it), ptr(mt), 200, L, None, ptr(pooled_g), int(mask.sum()),
                                             ptr(ws_g), need, ops.stream_ptr())
assert rc == 0, lib().gdr_last_error()
pooled_g.zero_()
graph.replay()
torch.cuda.synchronize()
out["digest"]["b200_graph"] = dg(pooled_g)
assert lib().gdr_device_fault_pending() == 0, lib().gdr_last_error()
print("RESULT " + json.dumps(out))
"""


def _run(chains):
    env = dict(os.environ, GDR_ENC_CHAINS=chains)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


@pytest.fixture(scope="module")
def runs():
    return _run("1"), _run("2")


CASES = ["b200", "b201", "b201_nohint", "b198", "b256_bench", "b200_uneven", "b200_holes"]


@pytest.mark.parametrize("case", CASES)
def test_two_chains_give_the_one_chain_bits(runs, case):
    one, two = runs
    assert two["digest"][case] == one["digest"][case], f"two chains changed the pooled output's bits at {case}"


def test_two_chains_are_taken_only_when_both_halves_pack(runs):
    one, two = runs
    # two chains: each half runs the whole launch sequence (pack plan, stream-K flags, every block, the CLS tail)
    for case in ["b200", "b201", "b256_bench", "b200_uneven", "b200_holes"]:
        assert two["launches"][case] == 2 * one["launches"][case], (case, one["launches"][case], two["launches"][case])
    # B = 198: a half of 99 x 40 rows is 186 tiles < 192: the call runs one chain
    assert two["launches"]["b198"] == one["launches"]["b198"] == one["launches"]["b200"]


def test_a_call_with_out_hidden_runs_one_chain(runs):
    one, two = runs
    assert two["launches"]["b200_hidden"] == one["launches"]["b200_hidden"]
    assert two["digest"]["b200_hidden_pooled"] == one["digest"]["b200_hidden_pooled"] == one["digest"]["b200"]


def test_workspace_of_the_stated_size_keeps_its_guard_bands_and_poison_does_not_matter(runs):
    one, two = runs                       # the bands are checked inside the child (abi_guard.Guard.check)
    for r in (one, two):
        assert r["digest"]["b200_guard_00"] == r["digest"]["b200_guard_ff"] == one["digest"]["b200"]
        assert r["one_byte_short_rc"] == -2, "a workspace one byte short must be refused (GDR_ENOSPC)"


def test_profiler_reports_the_union_of_overlapping_linears(runs):
    one, two = runs
    # per chain, 2 layers with the token table, pooled-only: block 0's o / wi / wo, the last block's k/v and CLS q, the CLS tail's
    # o / wi / wo
    assert one["prof"]["linear_launches"] == 8 and two["prof"]["linear_launches"] == 16
    for r in (one, two):
        assert 0.0 < r["prof"]["linear_ms"] <= r["prof"]["wall_ms"], r["prof"]


def test_captured_and_replayed_call_gives_the_one_chain_bits(runs):
    one, two = runs
    assert one["digest"]["b200_graph"] == one["digest"]["b200"]
    assert two["digest"]["b200_graph"] == one["digest"]["b200"]
