"""Appending GP training data: the host-side pieces that need no GPU.

* ``GaussianProcess.append_data`` followed by ``device_layout("cpu")`` gives the layout of a GP
  constructed on the concatenated data (d = 1 and d = 3).
* The ctypes signature table lists gpmpc_gp_reserve / gpmpc_gp_append / gpmpc_gp_size with the
  header's types, and misuse that needs no device (a null handle) is refused with GPMPC_ERR_ARG.
"""

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import gp_ref as R

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "gpmpc_mi355x.h"


def _gp(X, y, g):
    from gpmpc.gp import GaussianProcess

    gp = GaussianProcess(torch.tensor(X), torch.tensor(y))
    gp.set_hyperparameters(g["ell"], g["sf2"], g["sn2"])
    return gp


@pytest.mark.parametrize("d,n0,blocks", [(1, 13, (3, 16)), (3, 20, (7, 5, 1))])
def test_layout_after_append_equals_layout_of_concatenated_data(d, n0, blocks):
    n = n0 + sum(blocks)
    g = R.synthetic_gp(n, d, seed=5 + d)
    y = np.sin(g["X"].sum(1)) + 0.3
    gp = _gp(g["X"][:n0], y[:n0], g)
    first = gp.device_layout("cpu")   # cached: append_data must drop it
    assert first["n"] == n0
    at = n0
    for m in blocks:
        x = torch.tensor(g["X"][at:at + m])
        out = gp.append_data(x[:, 0] if d == 1 else x, torch.tensor(y[at:at + m]))
        assert out is gp and gp.K is None and gp.K_inv is None and gp._dev is None
        at += m
    assert gp.train_inputs[0].shape == (n, d) and gp.train_targets.shape == (n,) and gp.n_ind_points == n
    lay, want = gp.device_layout("cpu"), _gp(g["X"], y, g).device_layout("cpu")
    assert lay["n"] == want["n"] == n and lay["npad"] == want["npad"] and lay["d"] == d
    for key in ("rows", "linvT", "alpha", "Linv"):
        assert torch.equal(lay[key], want[key]), key
    with pytest.raises(ValueError):
        gp.append_data(torch.zeros(2, d + 1), torch.zeros(2))
    with pytest.raises(ValueError):
        gp.append_data(torch.zeros(2, d), torch.zeros(3))


C2CT = {"gpmpc_handle*": ctypes.c_void_p, "int32_t": ctypes.c_int32, "const double*": ctypes.c_void_p,
        "int32_t*": None, "void*": ctypes.c_void_p}


def _header_args(name):
    text = HEADER.read_text()
    m = re.search(r"gpmpc_status\s+" + name + r"\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in the header"
    return [re.sub(r"\s*\w+$", "", a.strip()) for a in m.group(1).replace("\n", " ").split(",")]


def test_signature_table_lists_the_new_entries_with_the_header_types():
    from gpmpc import _lib

    want = {"gpmpc_gp_reserve": ["gpmpc_handle*", "int32_t", "int32_t"],
            "gpmpc_gp_append": ["gpmpc_handle*", "int32_t", "int32_t", "const double*", "const double*", "int32_t*",
                                "void*"],
            "gpmpc_gp_size": ["gpmpc_handle*", "int32_t", "int32_t*", "int32_t*"]}
    for name, ctypes_c in want.items():
        assert _header_args(name) == ctypes_c, name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int32 and len(args) == len(ctypes_c), name
        for a, c in zip(args, ctypes_c):
            if c == "int32_t*":   # a device pointer (void*) or a host out-parameter
                assert a in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)), (name, a)
            else:
                assert a is C2CT[c], (name, c, a)


def test_null_handle_is_refused_without_a_device():
    from gpmpc import _lib

    if not _lib.LIB_PATH.exists():
        pytest.skip("library not built (run __graft_entry__.build())")
    lib = _lib.load(require_gpu=False)
    n, cap = ctypes.c_int32(-5), ctypes.c_int32(-5)
    for st in (lib.gpmpc_gp_reserve(None, 0, 32), lib.gpmpc_gp_append(None, 0, 1, None, None, None, None),
               lib.gpmpc_gp_size(None, 0, ctypes.byref(n), ctypes.byref(cap))):
        assert st == -1   # GPMPC_ERR_ARG
        assert b"null handle" in lib.gpmpc_last_error()
        with pytest.raises(_lib.GPMPCError, match="null handle"):
            _lib.check(st)
    assert (n.value, cap.value) == (-5, -5)
