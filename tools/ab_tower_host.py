"""Host-side A/B of the encoder towers between two builds of libgdr_hip.so, in a process without a GPU.

    python tools/ab_tower_host.py PARENT.so HEAD.so [OUT.json]

Loads both libraries side by side and compares, call by call:
  * the six tower *_workspace_bytes functions over a sweep of dims (several not multiples of 4 / 8 / 32 / 64 / 128) and of (B, L)
    (0, 1, T5_MAX_LEN - 1, T5_MAX_LEN, T5_MAX_LEN + 1 among them);
  * the nine tower forwards over a grid of refused calls — each pointer null in turn, each weight pointer null, B / L out of range, bad
    dims, bad `terms`, a workspace one byte short, a misaligned workspace, and every ordered pair of these faults — and over the
    well-formed call, which without a GPU fails at its first launch (GDR_EHIP): return code and gdr_last_error() text must be equal.
Device pointers are fake (never dereferenced by host code); the weight structs are real host memory.  Exit status 1 on any difference."""
import ctypes as C
import itertools
import json
import os
import sys

os.environ.setdefault("GDR_FFI_NO_TORCH", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gdr_amd import _ffi  # noqa: E402

FAKE = 0x7F0000000000  # a 256-byte aligned non-null "device" pointer
T5_MAX_LEN = 512


def load(path):
    l = C.CDLL(path, mode=os.RTLD_LOCAL | os.RTLD_NOW | getattr(os, "RTLD_DEEPBIND", 0))
    for name, (res, args) in _ffi.SIGNATURES.items():
        if name.startswith(("gdr_t5_encoder", "gdr_bert", "gdr_last_error")):
            fn = getattr(l, name)
            fn.restype, fn.argtypes = res, args
    return l


def t5_weights(d_model, d_kv, d_ff, H, layers=2):
    dims = _ffi.GdrT5Dims(64, d_model, d_kv, d_ff, H, layers, 32, 128, 1e-6)
    ly = (_ffi.GdrT5EncLayer * layers)()
    for x in ly:
        for f, _t in x._fields_:
            setattr(x, f, FAKE)
    return _ffi.GdrT5EncoderWeights(dims, FAKE, FAKE, FAKE, ly, None)


def bert_weights(d, H, d_ff, layers=2, max_pos=512):
    ly = (_ffi.GdrBertLayer * layers)()
    for x in ly:
        for f, _t in x._fields_:
            setattr(x, f, FAKE)
    return _ffi.GdrBertWeights(64, d, H, d_ff, layers, max_pos, 2, 1e-12, FAKE, FAKE, FAKE, FAKE, FAKE, ly)


# entry point -> (tower, its workspace function, argument order)
T5_PAD = ("w", "ids", "mask", "B", "L", "oh", "op", "ws", "wsb", "stream")
T5_RAG = ("w", "ids", "mask", "B", "L", "oh", "op", "hint", "ws", "wsb", "stream")
T5_SPL = ("w", "ids", "mask", "B", "L", "oh", "op", "hint", "terms", "ws", "wsb", "stream")
B_PAD = ("w", "ids", "mask", "tt", "B", "L", "oh", "op", "ws", "wsb", "stream")
B_RAG = ("w", "ids", "mask", "tt", "B", "L", "oh", "op", "hint", "ws", "wsb", "stream")
ENTRIES = {
    "gdr_t5_encoder_forward": ("t5", "gdr_t5_encoder_workspace_bytes", T5_PAD),
    "gdr_t5_encoder_forward_bf16": ("t5", "gdr_t5_encoder_bf16_workspace_bytes", T5_PAD),
    "gdr_t5_encoder_forward_ragged": ("t5", "gdr_t5_encoder_ragged_workspace_bytes", T5_RAG),
    "gdr_t5_encoder_forward_ragged_bf16": ("t5", "gdr_t5_encoder_ragged_workspace_bytes", T5_RAG),
    "gdr_t5_encoder_forward_ragged_split": ("t5", "gdr_t5_encoder_split_workspace_bytes", T5_SPL),
    "gdr_bert_encoder_forward": ("bert", "gdr_bert_encoder_workspace_bytes", B_PAD),
    "gdr_bert_encoder_forward_ragged": ("bert", "gdr_bert_encoder_ragged_workspace_bytes", B_RAG),
    "gdr_bert_encoder_forward_ragged_bf16": ("bert", "gdr_bert_encoder_ragged_workspace_bytes", B_RAG),
    "gdr_bert_encoder_forward_ragged_split": ("bert", "gdr_bert_encoder_ragged_workspace_bytes", B_RAG),
}

# a fault edits the call: `a` the arguments by name, `m` the model description the weight struct is made from.
# "short" / "misaligned" are applied to the workspace after its size is known.
COMMON = {
    "null w": lambda a, m: a.update(w=None),
    "null ids": lambda a, m: a.update(ids=None),
    "null mask": lambda a, m: a.update(mask=None),
    "null out_hidden": lambda a, m: a.update(oh=None),
    "null both outputs": lambda a, m: a.update(oh=None, op=None),
    "null workspace": lambda a, m: a.update(ws=None),
    "B = -1": lambda a, m: a.update(B=-1),
    "B = 0": lambda a, m: a.update(B=0),
    "L = 0": lambda a, m: a.update(L=0),
    "L = 513": lambda a, m: a.update(L=T5_MAX_LEN + 1),
    "workspace one byte short": lambda a, m: a.update(short=True),
    "workspace misaligned": lambda a, m: a.update(misaligned=True),
    "null layers": lambda a, m: m.update(null_field="layers"),
    "layer 1 null weight": lambda a, m: m.update(null_layer=1),
}
T5_FAULTS = dict(COMMON, **{
    "null embed": lambda a, m: m.update(null_field="embed"),
    "null rel_bias": lambda a, m: m.update(null_field="rel_bias"),
    "null final_ln": lambda a, m: m.update(null_field="final_ln"),
    "d_model = 770": lambda a, m: m.update(d=770),
    "d_model = 772": lambda a, m: m.update(d=772),
    "d_ff = 3074": lambda a, m: m.update(d_ff=3074),
    "d_ff = 3104": lambda a, m: m.update(d_ff=3104),
    "d_kv = 62": lambda a, m: m.update(d_kv=62),
    "d_kv = 32": lambda a, m: m.update(d_kv=32),
    "terms = 5": lambda a, m: a.update(terms=5),
    "terms = 2": lambda a, m: a.update(terms=2),
})
BERT_FAULTS = dict(COMMON, **{
    "null word_emb": lambda a, m: m.update(null_field="word_emb"),
    "null emb_ln_b": lambda a, m: m.update(null_field="emb_ln_b"),
    "null token types": lambda a, m: a.update(tt=None),
    "L > max_pos": lambda a, m: m.update(max_pos=8),
    "H = 0": lambda a, m: m.update(H=0),
    "d = 770": lambda a, m: m.update(d=770),
    "d = 192, H = 3": lambda a, m: m.update(d=192, H=3),
    "d = 96, H = 3": lambda a, m: m.update(d=96, H=3),
    "d_ff = 3074": lambda a, m: m.update(d_ff=3074),
    "d_ff = 3104": lambda a, m: m.update(d_ff=3104),
})
# (model, B, L): one shape per route of the dispatchers (padded fallback, small, big / two chains, above 128 tokens)
T5_SHAPES = [(dict(d=768, d_kv=64, d_ff=3072, H=12), B, L) for B, L in ((8, 16), (64, 40), (512, 40), (16, 300))] + \
            [(dict(d=512, d_kv=64, d_ff=2048, H=8), 96, 128), (dict(d=64, d_kv=64, d_ff=128, H=1), 4, 64)]
BERT_SHAPES = [(dict(d=768, H=12, d_ff=3072, max_pos=512), B, L) for B, L in ((8, 16), (64, 128), (8, 512))] + \
              [(dict(d=128, H=2, d_ff=128, max_pos=512), 4, 32)]


def call(lib, entry, model, B, L, faults, table):
    tower, ws_fn, order = ENTRIES[entry]
    m = dict(model)
    a = dict(w=True, ids=FAKE, mask=FAKE, tt=FAKE, B=B, L=L, oh=FAKE, op=FAKE, hint=-1, terms=6, ws=FAKE, stream=None)
    for f in faults:
        table[f](a, m)
    if tower == "t5":
        w = t5_weights(m["d"], m["d_kv"], m["d_ff"], m["H"])
        size_arg = C.byref(w.dims)
    else:
        w = bert_weights(m["d"], m["H"], m["d_ff"], max_pos=m["max_pos"])
        size_arg = C.byref(w)
    if m.get("null_field") == "layers":
        w.layers = C.POINTER(type(w.layers.contents))()
    elif m.get("null_field"):
        setattr(w, m["null_field"], None)
    if "null_layer" in m and w.layers:
        w.layers[m["null_layer"]].wi = None
    need = getattr(lib, ws_fn)(size_arg, a["B"], a["L"])
    a["wsb"] = need - 1 if a.get("short") and need else need
    if a.get("misaligned") and a["ws"]:
        a["ws"] = FAKE + 8
    a["w"] = C.byref(w) if a["w"] else None
    rc = getattr(lib, entry)(*[a[k] for k in order])
    return rc, lib.gdr_last_error().decode("utf-8", "replace") if rc else ""


def main():
    parent, head = load(sys.argv[1]), load(sys.argv[2])
    addr = lambda l: C.cast(l.gdr_t5_encoder_forward, C.c_void_p).value
    assert addr(parent) != addr(head), "the two paths loaded as one library"
    bad = []
    # ---- sizes
    n_sizes = 0
    widths = [(768, 64, 3072, 12), (512, 64, 2048, 8), (1024, 64, 4096, 16), (64, 64, 128, 1), (256, 64, 512, 4), (770, 62, 3074, 12),
              (772, 60, 3076, 5), (96, 32, 100, 3), (36, 12, 20, 3), (1000, 40, 1500, 25), (4, 4, 4, 1), (7, 3, 5, 1), (768, 64, 3072, 1)]
    shapes = [(B, L) for B in (-1, 0, 1, 2, 3, 7, 64, 96, 97, 191, 192, 193, 512, 1000) for L in (0, 1, 2, 16, 40, 127, 128, 129, 300,
                                                                                                T5_MAX_LEN - 1, T5_MAX_LEN, T5_MAX_LEN + 1)]
    for (d, dk, dff, H), (B, L) in itertools.product(widths, shapes):
        tw, bw = t5_weights(d, dk, dff, H), bert_weights(d, H, dff)
        for fn, arg in [(f, C.byref(tw.dims)) for f in ("gdr_t5_encoder_workspace_bytes", "gdr_t5_encoder_bf16_workspace_bytes",
                                                        "gdr_t5_encoder_ragged_workspace_bytes", "gdr_t5_encoder_split_workspace_bytes")] + \
                       [(f, C.byref(bw)) for f in ("gdr_bert_encoder_workspace_bytes", "gdr_bert_encoder_ragged_workspace_bytes")]:
            p, h = getattr(parent, fn)(arg, B, L), getattr(head, fn)(arg, B, L)
            n_sizes += 1
            if p != h:
                bad.append(("size", fn, (d, dk, dff, H), B, L, p, h))
    # ---- calls
    n_refused = n_reached = n_ok = 0
    by_rc, reached = {}, {}
    for entry, (tower, _ws_fn, _order) in ENTRIES.items():
        table = T5_FAULTS if tower == "t5" else BERT_FAULTS
        names = list(table)
        grids = [()] + [(f,) for f in names] + list(itertools.permutations(names, 2))
        for (model, B, L), faults in itertools.product(T5_SHAPES if tower == "t5" else BERT_SHAPES, grids):
            p, h = call(parent, entry, model, B, L, faults, table), call(head, entry, model, B, L, faults, table)
            if p != h:
                bad.append(("call", entry, model, B, L, faults, p, h))
            by_rc[p[0]] = by_rc.get(p[0], 0) + 1
            if p[0] == _ffi.GDR_EHIP:
                n_reached += 1
                reached[entry] = reached.get(entry, set()) | {p[1]}
            elif p[0] == 0:
                n_ok += 1
            else:
                n_refused += 1
    out = {"sizes_compared": n_sizes, "calls_refused_compared": n_refused, "calls_reaching_first_launch_compared": n_reached,
           "calls_returning_ok_compared": n_ok, "parent_return_codes": {str(k): v for k, v in sorted(by_rc.items())},
           "first_launch_failures": {k: sorted(v) for k, v in reached.items()}, "differences": len(bad), "first_differences": [repr(b) for b in bad[:20]]}
    print(json.dumps(out, indent=1))
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
