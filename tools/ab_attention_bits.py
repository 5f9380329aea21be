"""Every attention form of launch_attention (csrc/attention.hip, csrc/attention_long.hip) on fixed synthetic inputs, for comparing two
builds of libgdr_hip.so bit for bit on one GPU — one process per library, the Python files being the same:

    GDR_HIP_LIB=/path/to/parent/libgdr_hip.so timeout -k 10 600 python tools/ab_attention_bits.py --out parent.json \
        && timeout -k 10 600 python tools/ab_attention_bits.py --out head.json \
        && python tools/ab_attention_bits.py --compare parent.json head.json

A run records, per call, the sha256 of all output bytes and the library's launch count (gdr_launch_count); --compare (no GPU) prints the
calls whose digest or count differ and exits 1 if there is one.  Under `rocprofv3 --kernel-trace --stats -- python tools/ab_attention_bits.py
--out x.json` the same run lists the kernels reached: every attention kernel template appears (the shapes below are the smallest that
reach each form and each tile-count edge).

Models: the small shape of tests/peaked.py (d_model 128, d_kv 64, 4 heads, d_ff 256, 2 layers; 19 output positions, so that a decode
step sees 1 .. 18 cached keys) and variants of it — d_kv 32 (the generic kernel), d_model 256 (the decode cross-attention reads its q rows
as split-K slabs), an adaptor of one 128-wide head (the 32-lanes-per-row decode forms) — and the tiny doc tower (2 heads of 64)."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = 19
CFG64 = dict(d_model=128, d_kv=64, num_heads=4, d_ff=256, max_output_length=STEPS, decode_vocab_size=6 * STEPS + 2)
ENC_L = (1, 16, 17, 33, 40, 64, 80, 96, 112, 128)   # 16-key tiles 1, 1, 2, 3, 3, 4, 5, 6, 7, 8
LONG_L = (129, 200, 512)


def lengths(L, B=6):
    """B sequence lengths mixed down to 1, the first of them L."""
    return [max(1, (L * (B - i)) // B) for i in range(B - 1)] + [1]


def tokens(lens, L, vocab, seed, dead_row=False):
    g = np.random.Generator(np.random.PCG64(seed))
    lens = np.asarray(lens)
    ids = g.integers(2, vocab, size=(len(lens), L)).astype(np.int64)
    mask = (np.arange(L)[None, :] < lens[:, None]).astype(np.int64)
    ids[np.arange(len(lens)), lens - 1] = 1
    if dead_row:   # one fully masked row: it attends uniformly over its PAD keys
        mask = np.concatenate([mask, np.zeros((1, L), np.int64)])
        ids = np.concatenate([ids, np.zeros((1, L), np.int64)])
    return ids * mask, mask


def run(out_path):
    import torch
    from gdr_amd import _ffi, ops, synth
    from gdr_amd.config import GDRConfig
    from gdr_amd.modeling import EncoderModel
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    count = _ffi.lib().gdr_launch_count
    out = {}

    def call(name, fn):
        n0 = count()
        try:
            res = fn()
            res = res if isinstance(res, (tuple, list)) else (res,)
            h = hashlib.sha256()
            for t in res:
                if t is not None:
                    h.update(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())
            digest = h.hexdigest()
        except (_ffi.GdrError, ValueError) as e:   # a refusal (GDR_EINVAL, or the Python layer's): its text is compared
            if isinstance(e, _ffi.GdrError) and "(code -1)" not in str(e) and "split=True" not in str(e):
                raise                              # a HIP error is no refusal: the run ends here
            res, digest = None, "refused: " + str(e)
        torch.cuda.synchronize()
        out[name] = [digest, int(count() - n0)]
        return res

    def d(a):
        return torch.from_numpy(a).to(dev)

    # ---- T5 encoder: fp32, bf16 mode, split; padded and ragged; d_kv 64 and 32; up to 128 tokens and above
    for tag, over in (("dkv64", CFG64), ("dkv32", dict(CFG64, d_kv=32))):
        cfg = GDRConfig.tiny(**over)
        sd = synth.make_state_dict(cfg, seed=401, with_decoder=False)
        handles = {"f32": ops.T5EncoderHandle(cfg, sd, dev), "bf16": ops.T5EncoderHandle(cfg, sd, dev, dtype=torch.bfloat16),
                   "split": ops.T5EncoderHandle(cfg, sd, dev, split=True)}
        for L in (ENC_L + LONG_L) if tag == "dkv64" else (40, 128, 129, 512):
            ids, mask = tokens(lengths(L), L, cfg.vocab_size, 1000 + L, dead_row=True)
            it, mt = d(ids), d(mask)
            for hname, enc in handles.items():
                if hname != "split":
                    call(f"enc/{tag}/{hname}/L{L}/padded", lambda: enc.forward(it, mt))
                call(f"enc/{tag}/{hname}/L{L}/ragged", lambda: enc.forward(it, mt, ragged=True, live_rows_hint=int(mask.sum())))
        del handles

    # ---- doc tower (scale 1/8, no position bias): fp32 padded and ragged, bf16 mode; the ragged forms also on a batch past bert.hip's
    #      packed-kernel threshold (192 GEMM tiles of 128 token rows)
    bc = dict(synth.bert_config(True), max_pos=512)
    bsd = synth.make_bert_state_dict(bc, seed=402)
    for hname, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        tower = EncoderModel.from_state_dict(bc, bsd, dev, dtype=dt).bert
        for L in (1, 17, 40, 100, 128) + LONG_L:
            ids, mask = tokens(lengths(L, 8), L, bc["vocab_size"], 2000 + L, dead_row=True)
            it, mt = d(ids), d(mask)
            if hname == "f32":
                call(f"bert/{hname}/L{L}/padded", lambda: tower.forward(it, mt, ragged=False))
            call(f"bert/{hname}/L{L}/ragged", lambda: tower.forward(it, mt, ragged=True, live_rows_hint=int(mask.sum())))
        for L in (100, 200):
            ids, mask = tokens(lengths(L, 8), L, bc["vocab_size"], 2000 + L)
            reps = -(-(192 * 128) // ids.size)
            it, mt = d(np.tile(ids, (reps, 1))), d(np.tile(mask, (reps, 1)))
            call(f"bert/{hname}/L{L}/ragged x{reps}", lambda: tower.forward(it, mt, ragged=True, live_rows_hint=int(mask.sum()) * reps))
        del tower

    # ---- generate() and score(): 1, 2, 17 and 30 beams over encoder lengths on both sides of every form's edge; 18 decode steps
    def decode_cases(tag, over, shapes, precisions=("f32", "bf16"), seed=403):
        cfg = GDRConfig.tiny(**over)
        sd = synth.make_state_dict(cfg, seed=seed)
        for pname in precisions:
            dt = torch.bfloat16 if pname == "bf16" else torch.float32
            enc = ops.T5EncoderHandle(cfg, sd, dev, dtype=dt)
            dec = ops.T5DecoderHandle(cfg, sd, dev, dtype=dt)
            for B, R, L in shapes:
                ids, mask = tokens(lengths(L, B) if B > 1 else [L], L, cfg.vocab_size, 3000 + 7 * L + R)
                it, mt = d(ids), d(mask)
                states, _ = enc.forward(it, mt, want_pooled=False, ragged=True)
                res = call(f"generate/{tag}/{pname}/B{B}xR{R}/L{L}", lambda: dec.generate(states, mt, R, STEPS, 0.8, R))
                if res is not None and R > 1 and B <= 8:   # teacher forcing over the rows just decoded, with the hidden-state outputs
                    call(f"score/{tag}/{pname}/B{B}xR{R}/L{L}", lambda: dec.score(states, mt, res[0], R, 0.8, hidden=True))
            del enc, dec

    decode_cases("dkv64", CFG64, [(5, R, L) for R in (1, 2, 17, 30) for L in (5, 40, 128, 129, 512)] +
                 [(5, 17, L) for L in (17, 64, 80, 96, 112)])                 # the beam-row MFMA form's tile counts 2, 4, 5, 6, 7
    decode_cases("dkv64/heads4", CFG64, [(137, 30, 12)])                      # 137 x 30 rows x 4 heads >= 16 384: four heads per wave
    decode_cases("dkv32", dict(CFG64, d_kv=32), [(5, 17, 40), (5, 17, 129)], ("f32",))
    decode_cases("dmodel256", dict(CFG64, d_model=256), [(3, 6, 40), (3, 6, 300), (3, 1, 300)])   # slab-sourced q rows
    decode_cases("adaptor128", dict(CFG64, adaptor_nhead=1), [(5, 6, 40)], ("f32",))              # 32 lanes per K / V row

    with open(out_path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print(f"{len(out)} calls, {sum(v[1] for v in out.values())} kernel launches, "
          f"{sum(1 for v in out.values() if v[0].startswith('refused'))} refused -> {out_path}")


def compare(pa, pb):
    a, b = json.load(open(pa)), json.load(open(pb))
    bad = 0
    if set(a) != set(b):
        print("different sets of calls:", sorted(set(a) ^ set(b)))
        bad = 1
    names = sorted(set(a) & set(b))
    bits = [n for n in names if a[n][0] != b[n][0]]
    launches = [n for n in names if a[n][1] != b[n][1]]
    refused = [n for n in names if a[n][0].startswith("refused")]
    print(f"calls compared {len(names)} (sha256 of all output bytes; {len(refused)} of them refused, the text compared)")
    print(f"calls with different output bytes {len(bits)}")
    print(f"calls with a different launch count {len(launches)}")
    print(f"kernel launches per run: {sum(a[n][1] for n in names)} / {sum(b[n][1] for n in names)}")
    for n in bits:
        print("  bytes differ:", n, a[n][0][:16], b[n][0][:16])
    for n in launches:
        print("  launches differ:", n, a[n][1], b[n][1])
    print("\n# call : launches (equal in both), sha256[:16]")
    for n in names:
        if n not in bits and n not in launches:
            print(f"{n} : {a[n][1]} {a[n][0][:16] if not a[n][0].startswith('refused') else a[n][0]}")
    return 1 if (bad or bits or launches) else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    run(args.out)
