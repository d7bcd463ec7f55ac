"""The flow-program compiler's routes, pinned: which row width, how many launches, which ops with which fields and how
many parameter floats each preset compiles to (tests/golden/program_routes.json, written by
``tools/program_fingerprint.py --routes``; the parameter bytes themselves are compared by that tool between two commits on
one machine), and the op codes of torchflows_amd/flow_ops.py against include/tfk.h.  No GPU needed: the programs are
packed on the host."""
import functools
import importlib.util
import json
import os
import re

import pytest
import torch

from conftest import GOLDEN, ROOT


def _tool():
    spec = importlib.util.spec_from_file_location("program_fingerprint", os.path.join(ROOT, "tools", "program_fingerprint.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _tool()
with open(os.path.join(GOLDEN, "program_routes.json")) as _f:
    CASES = json.load(_f)["cases"]


@functools.lru_cache(maxsize=None)
def _flow(case):
    return TOOL.build_flow(case)


# the row-width classes each preset reaches on the grid of the tool, without / with a context: what the fixture must cover
_AFFINE = ({"16", "32", "64", "128", "256", "wide"}, {"64", "128", "256", "declined"})
_SPLINE = ({"32", "64", "128", "256", "declined"}, {"64", "128", "256", "declined"})
_MADE = ({"32", "64", "128", "256", "declined"}, {"declined"})
_MADE_SPLINE = ({"64", "128", "declined"}, {"declined"})
COVERAGE = {"RealNVP": _AFFINE, "NICE": _AFFINE, "CouplingRQNSF": _SPLINE, "CouplingLRS": _SPLINE, "MAF": _MADE, "IAF": _MADE,
            "MaskedAutoregressiveRQNSF": _MADE_SPLINE, "InverseAutoregressiveRQNSF": _MADE_SPLINE,
            "MaskedAutoregressiveLRS": _MADE_SPLINE}


def test_route_fixture_covers_the_grid():
    """A case for every (preset, row-width class, context) combination of the grid, and the boundary chains."""
    assert set(COVERAGE) == set(TOOL.PRESETS)
    got = {(c["preset"], TOOL.width_class(c["expect"]), bool(c["context"])) for c in CASES
           if c["n_layers"] == 3 and c["n_hidden"] is None}
    want = {(p, w, ctx) for p, classes in COVERAGE.items() for ctx in (False, True) for w in classes[ctx]}
    assert got == want
    boundary = {(c["preset"], c["D"], c["n_layers"], c["n_hidden"]) for c in CASES}
    assert boundary >= set(TOOL.BOUNDARY)


def test_old_spelling_of_the_compiler_entry_points():
    """``fused._flatten`` / ``_compile_lean`` / ``_lean_coupling`` (earlier releases) are flow_compile's functions."""
    from torchflows_amd import flow_compile, fused
    for name in ("_flatten", "_compile_lean", "_lean_coupling"):
        assert getattr(fused, name) is getattr(flow_compile, name)
    with pytest.raises(AttributeError):
        fused._pack_lean


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_program_route(case, monkeypatch):
    from torchflows_amd import fused
    monkeypatch.delenv("TORCHFLOWS_AMD_DEBUG", raising=False)
    monkeypatch.delenv("TORCHFLOWS_AMD_MFMA", raising=False)
    monkeypatch.delenv("TORCHFLOWS_AMD_FUSED", raising=False)
    flow = _flow((case["preset"], case["D"], case["context"], case["n_layers"], case["n_hidden"]))
    chain = fused.compile_chain(flow.bijection, case["direction"], torch.device("cpu"), context=bool(case["context"]))
    assert TOOL.describe(chain, sha=False) == case["expect"]


def test_op_codes_match_the_header():
    """flow_ops.OP_* are the enumerators TFK_OP_* of include/tfk.h, all of them, with the same values."""
    from torchflows_amd import flow_ops
    with open(os.path.join(ROOT, "include", "tfk.h")) as f:
        header = dict((name, int(value)) for name, value in re.findall(r"^\s*TFK_OP_(\w+)\s*=\s*(\d+)", f.read(), re.M))
    ours = {name[3:]: getattr(flow_ops, name) for name in dir(flow_ops) if name.startswith("OP_")}
    assert len(header) == 29 and ours == header
    assert flow_ops.LEAN_BY_OP.keys() <= set(header.values())
    for kind in flow_ops.LEAN_KINDS.values():
        assert [n for n, v in header.items() if v == kind.op][0].endswith("_LEAN")
