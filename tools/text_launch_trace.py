#!/usr/bin/env python3
"""The launch trace of a step, on the CPU against a stub library that computes nothing: every medmoe_* launch of one train_step (for some
cases also one eval_step after it) on oracle config tiny2, with ALL its arguments - integers and floats as they are, every pointer as the
long-lived buffer it points into plus a byte offset (`ws.tqkv+0`, `tstore.p16t+8192`, `text.layer.0.attention_layernorm.weight+0`,
`base_t.layer.1.feedforward.model.0.weight+0`), `null`, or `tmp` for anything else.  tests/test_text_launch_trace_host.py compares the
SHA-256 of every case's trace with tests/golden/text_launch_digests.json: a change to engine.py that is meant to keep the launches keeps the
digests.

    python tools/text_launch_trace.py                    # case, launch count, digest
    python tools/text_launch_trace.py --dump CASE        # the trace itself, one launch per line (diff two commits' dumps to find a change)
    python tools/text_launch_trace.py --record           # rewrite the golden file (only for a change that alters the launches on purpose)
"""
import argparse
import bisect
import contextlib
import ctypes
import hashlib
import importlib.util
import json
import os
import sys
from unittest import mock

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
GOLDEN = os.path.join(ROOT, "tests", "golden", "text_launch_digests.json")

FULL, LORA = dict(freeze_text=False), dict(text_lora=True, text_lora_r=8)
SHALLOW = dict(n_layer_t=2, last_n_layers=4)          # the embedding output is among the summed states
# case -> (config overrides, environment, also trace an eval_step after the train_step)
CASES = {
    "frozen-packed": ({}, {}, False),
    "frozen-padded": ({}, {"MEDMOE_TEXT_VARLEN": "0"}, False),
    "frozen-last1": (dict(last_n_layers=1), {}, False),
    "frozen-shallow": (SHALLOW, {}, False),
    "full-padded+eval": (FULL, {}, True),
    "full-padded-hidden-attn-drop": (dict(FULL, text_hidden_dropout=0.1, text_attn_dropout=0.1), {}, False),
    "full-padded-attn-drop": (dict(FULL, text_attn_dropout=0.1), {}, False),
    "full-packed-hidden-drop+eval": (dict(FULL, text_train_varlen=True, text_hidden_dropout=0.1), {}, True),
    "full-packed": (dict(FULL, text_train_varlen=True), {}, False),
    "full-last1": (dict(FULL, last_n_layers=1), {}, False),
    "full-shallow": (dict(FULL, **SHALLOW), {}, False),
    "lora-padded-all-drop": (dict(LORA, text_lora_dropout=0.1, text_hidden_dropout=0.1, text_attn_dropout=0.1), {}, False),
    "lora-padded+eval": (LORA, {}, True),
    "lora-packed-lora-drop+eval": (dict(LORA, text_train_varlen=True, text_lora_dropout=0.1), {}, True),
    "lora-packed-hidden-drop": (dict(LORA, text_train_varlen=True, text_hidden_dropout=0.1), {}, False),
    "lora-shallow": (dict(LORA, **SHALLOW), {}, False),
}
_ENV = ("MEDMOE_TEXT_VARLEN", "MEDMOE_TEXT_TRAIN_VARLEN", "MEDMOE_GRAPH", "MEDMOE_DETERMINISTIC", "MEDMOE_GRAD_COMM", "MEDMOE_OVERLAP_WGRAD",
        "MEDMOE_WGRAD_STAGED", "MEDMOE_LOCAL_PAIR3", "MEDMOE_LOCAL_GRAM", "MEDMOE_PAIR_PITCH", "MEDMOE_DIST_WORLD1")
_HOST_QUERIES = ("medmoe_local_geometry", "medmoe_local_fast_path", "medmoe_local_pair3_supported")     # and every *_scratch size
_FLAT = ("p32", "g32", "p16", "p16t", "m", "v", "e32", "_g16", "normsq", "norm_scratch", "tr_table")


def _stub_class():
    spec = importlib.util.spec_from_file_location("_text_varlen_train_host", os.path.join(ROOT, "tests", "test_text_varlen_train_host.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod._StubLib


class _TraceLib(_stub_class()):
    """The stub library, keeping every launch's arguments too (while `eng` is set).  One function object per entry point, so that the
    argument types ops.py declares on it are there to tell a pointer from an integer when plain Python values arrive."""

    def __init__(self):
        super().__init__()
        self.eng, self.trace, self._fns = None, [], {}

    def __getattr__(self, name):
        stub = super().__getattr__(name)
        fn = self._fns.get(name)
        if fn is None:
            def fn(*a):
                if self.eng is not None and name not in _HOST_QUERIES and not name.endswith("_scratch"):
                    self.trace.append(name + "(" + ", ".join(self._args(a, getattr(fn, "argtypes", None))) + ")")
                return stub(*a)
            self._fns[name] = fn
        return fn

    def _args(self, args, argtypes):
        names = _name_map(self.eng)
        out = []
        for i, a in enumerate(args[:-1]):                                     # the last argument is the stream
            if isinstance(a, ctypes.c_void_p):
                out.append(names(a.value))
            elif isinstance(a, ctypes._SimpleCData):
                out.append(repr(a.value))
            elif argtypes is None:
                raise TypeError(f"argument {i} = {a!r} arrives as a plain value at an entry point without declared argument types")
            elif argtypes[i] is ctypes.c_void_p:
                out.append(names(a))
            else:
                out.append(repr(a))
        return out


def _name_map(eng):
    """pointer -> name+offset over the buffers that are alive NOW (built per launch: an address is only ever attributed to a tensor that
    holds it at that moment, never to one that was freed).  In order of precedence: the workspace, the stores' flat buffers, the entries of
    params.text (views of a trainable tower's flat buffers resolve to those), the LoRA base's transposes."""
    named = [("ws." + k, v) for k, v in eng.ws.items()]
    for label, store in (("params", eng.params), ("tstore", eng.tstore), ("lora", eng.lora)):
        if store is not None:
            named += [(f"{label}.{k}", getattr(store, k, None)) for k in _FLAT]
    named += [("text." + k, v) for k, v in eng.params.text.items()]
    named += [("base_t." + k, v[1]) for k, v in eng._base_t.items()]
    starts, spans = [], []
    for name, t in named:
        if t is None or t.numel() == 0:
            continue
        lo = t.data_ptr()
        i = bisect.bisect_right(starts, lo)
        if i and lo < spans[i - 1][0]:                                        # inside a buffer of higher precedence
            continue
        starts.insert(i, lo); spans.insert(i, (lo + t.numel() * t.element_size(), name))

    def resolve(p):
        if not p:
            return "null"
        i = bisect.bisect_right(starts, p)
        return f"{spans[i - 1][1]}+{p - starts[i - 1]}" if i and p < spans[i - 1][0] else "tmp"
    return resolve


@contextlib.contextmanager
def _installed(lib, env):
    """What the `stub` fixture of the host tests patches, and the case's environment."""
    import torch
    from medmoe_amd import _lib, ops
    with contextlib.ExitStack() as es:
        es.enter_context(mock.patch.dict(os.environ, env))
        for k in _ENV:
            if k not in env:
                os.environ.pop(k, None)
        for obj, attr, val in ((_lib, "_LIB", lib), (ops, "load_library", lambda: lib), (ops, "_require_gpu", lambda t, name: None),
                               (ops, "_stream", lambda: ctypes.c_void_p(0)), (ops, "_stream_handle", lambda: 0),
                               (ops, "_FN", {}), (ops, "_NT_FN", {}), (ops, "_TN_FN", {}),
                               (torch.cuda, "is_available", lambda: True), (torch.cuda, "set_device", lambda d: None)):
            es.enter_context(mock.patch.object(obj, attr, val))
        yield


def trace(case: str):
    """The launches of `case` in a fresh engine: a list of strings."""
    import medmoe_oracle as O
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    overrides, env, with_eval = CASES[case]
    lib = _TraceLib()
    with _installed(lib, env):
        cfg = config_by_name("tiny2")
        for k, v in overrides.items():
            setattr(cfg, k, v)
        eng = Engine(cfg, "cpu")
        batch = O.synthetic_batch(O.config_by_name("tiny2"), 8, min_len=4)
        lib.eng = eng
        eng.train_step(batch)
        if with_eval:
            eng.eval_step(batch)
    return lib.trace


def digest(case: str):
    t = trace(case)
    return {"sha256": hashlib.sha256("\n".join(t).encode()).hexdigest(), "launches": len(t)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--dump", metavar="CASE", choices=list(CASES))
    ap.add_argument("--record", action="store_true", help="write the digests of every case to " + os.path.relpath(GOLDEN, ROOT))
    a = ap.parse_args()
    if a.dump:
        print("\n".join(trace(a.dump)))
        return
    got = {case: digest(case) for case in CASES}
    for case, d in got.items():
        print(f"{case:34s} {d['launches']:4d}  {d['sha256']}")
    if a.record:
        with open(GOLDEN, "w") as f:
            json.dump(got, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
