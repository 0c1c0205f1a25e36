"""Record the layout of every flat parameter store (ParamStore, TextStore, FlatStore) at small configurations: per store numel, the ordered
offsets, shapes, the transpose table and, for every name and every accessor that applies to it, the view's shape and storage offset.
Runs on the CPU against the stub library of tests/test_host_logic.py (no launch computes anything; the layout is host arithmetic).

    python tools/record_store_layouts.py > tests/golden/store_layouts.json

tests/test_host_logic.py::test_store_layouts_are_the_recorded_ones rebuilds the same stores and compares them with that file."""
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SWIN_TINY = dict(depths=(1, 1), heads=(1, 2), embed_dim=32, image_size=56)      # the smallest geometry SwinTower accepts: two stages, one block each


def swin_tiny_weights():
    """name -> zeros of the SwinModel state_dict shapes at SWIN_TINY (floating parameters, state_dict order)."""
    w = {}
    E = SWIN_TINY["embed_dim"]
    w["embeddings.patch_embeddings.projection.weight"] = (E, 3, 4, 4); w["embeddings.patch_embeddings.projection.bias"] = (E,)
    w["embeddings.norm.weight"] = (E,); w["embeddings.norm.bias"] = (E,)
    n_stage = len(SWIN_TINY["depths"])
    for s, depth in enumerate(SWIN_TINY["depths"]):
        C = E * 2 ** s
        for i in range(depth):
            pre = f"encoder.layers.{s}.blocks.{i}."
            for n in ("q_proj", "k_proj", "v_proj", "o_proj"):
                w[pre + f"attention.{n}.weight"] = (C, C); w[pre + f"attention.{n}.bias"] = (C,)
            w[pre + "attention.relative_position_bias.relative_position_bias_table"] = (169, SWIN_TINY["heads"][s])
            for n in ("layernorm_before", "layernorm_after"):
                w[pre + n + ".weight"] = (C,); w[pre + n + ".bias"] = (C,)
            w[pre + "mlp.fc1.weight"] = (4 * C, C); w[pre + "mlp.fc1.bias"] = (4 * C,)
            w[pre + "mlp.fc2.weight"] = (C, 4 * C); w[pre + "mlp.fc2.bias"] = (C,)
        if s + 1 < n_stage:
            pre = f"encoder.layers.{s}.downsample."
            w[pre + "reduction.weight"] = (2 * C, 4 * C); w[pre + "norm.weight"] = (4 * C,); w[pre + "norm.bias"] = (4 * C,)
    C = E * 2 ** (n_stage - 1)
    w["layernorm.weight"] = (C,); w["layernorm.bias"] = (C,)
    return {k: torch.zeros(s) for k, s in w.items()}


def build_stores():
    """label -> store, on the CPU."""
    from medmoe_amd.config import config_by_name
    from medmoe_amd.flat import FlatStore
    from medmoe_amd.params import ParamStore
    from medmoe_amd.pyramid import GroupedPyramidExperts
    from medmoe_amd.swin import SwinTower
    from medmoe_amd.text_params import TextStore
    out = {}
    for name in ("tiny", "tiny2", "tinyL8", "tinyL8mx"):
        out[f"ParamStore:{name}"] = ParamStore(config_by_name(name), "cpu")
    out["TextStore:tiny"] = TextStore(config_by_name("tiny"), "cpu", out["ParamStore:tiny"].text)
    # the grouped pyramid experts' arena of tests/test_parity2_gpu.py::test_grouped_pyramid_experts_reference_fixture
    z = np.load(os.path.join(ROOT, "tests", "golden", "expert_pyramid_mfma.npz"))
    E = 3
    allw = {f"moe.experts.{e}.{k}": torch.from_numpy(z[k]) for e in range(E) for k in z.files if k.startswith(("proj_convs", "attn_proj"))}
    gemm = [f"moe.experts.{e}.proj_convs.{s}.0.weight" for e in range(E) for s in range(4)] + [f"moe.experts.{e}.attn_proj.0.weight" for e in range(E)]
    out["FlatStore:grouped-pyramid"] = FlatStore(allw, "cpu", groups=GroupedPyramidExperts.groups(E), gemm=gemm)
    out["FlatStore:swin-tiny"] = SwinTower(swin_tiny_weights(), "cpu", **SWIN_TINY).store
    return out


def describe(st):
    """The layout of one store as plain JSON data.  entries: in the order of `offsets`, [name, offset, shape, distinct views, accessors]:
    a view is [shape, storage offset]; `accessors` has one character per accessor in the order f32, grad, w16, w16t, grad2d - the index of
    that accessor's view among the distinct ones, or "-" where the accessor does not apply: the spec-built stores (ParamStore, TextStore)
    read w16 of every name and w16t of their GEMM weights; a FlatStore has w16 / w16t / grad2d for its GEMM weights only."""
    spec_built = hasattr(st, "kinds")
    gemm = {n for n in st.shapes if st.kinds[n] == "wt"} if spec_built else set(st._mat)
    applies = {"f32": lambda n: True, "grad": lambda n: True, "w16": lambda n: spec_built or n in gemm, "w16t": lambda n: n in gemm,
               "grad2d": lambda n: not spec_built and n in gemm}
    assert set(st.offsets) == set(st.shapes)
    entries = []
    for n, o in st.offsets.items():
        distinct, code = [], ""
        for acc, ok in applies.items():
            if not ok(n):
                code += "-"
                continue
            v = getattr(st, acc)(n)
            v = [list(v.shape), v.storage_offset()]
            if v not in distinct:
                distinct.append(v)
            code += str(distinct.index(v))
        entries.append([n, o, list(st.shapes[n]), distinct, code])
    return {"numel": st.numel, "entries": entries, "tr_table": None if st.tr_table is None else st.tr_table.tolist(),
            "tr_max_tiles": st.tr_max_tiles}


def record():
    """label -> description; a store whose description equals an earlier one's is recorded as {"same_as": that label}."""
    out = {}
    for label, st in build_stores().items():
        d = describe(st)
        same = next((k for k, v in out.items() if v == d), None)
        out[label] = d if same is None else {"same_as": same}
    return out


def main():
    for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    from test_host_logic import _StubLib
    from medmoe_amd import _lib, ops
    lib = _StubLib()
    _lib._LIB = lib
    ops.load_library = lambda: lib
    ops._require_gpu = lambda t, name: None
    ops._stream = lambda: ctypes.c_void_p(0)
    ops._stream_handle = lambda: 0
    json.dump(record(), sys.stdout, separators=(",", ":"))
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
