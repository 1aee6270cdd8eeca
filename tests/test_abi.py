"""CPU checks of the C-ABI boundary: libfdr.so loads and exports every symbol include/fdr.h (the drop-in boundary)
and include/fdr_diag.h (diagnostics outside it) declare."""
import ctypes
import os
import re

import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "fdr.h")
DIAG = os.path.join(REPO, "include", "fdr_diag.h")


def declared_functions(headers=(HEADER, DIAG)):
    out = set()
    for h in headers:
        src = re.sub(r"/\*.*?\*/", "", open(h).read(), flags=re.S)
        out |= set(re.findall(r"\b(fdr_[a-z0-9_]+)\s*\(", src))
    return sorted(out)


def test_boundary_header_carries_no_diagnostics():
    """the A/B setters of the pruned kernel forms are gone, and the measurement hooks (phase
    profile, debug clocks, replay switch) live in fdr_diag.h, outside the drop-in boundary."""
    names = declared_functions((HEADER,))
    for gone in ("fdr_ctx_set_core_mfma", "fdr_ctx_set_conv_h2"):
        assert gone not in declared_functions()
    for diag in ("fdr_impala_debug_clock", "fdr_ctx_impala_debug_clock", "fdr_impala_profile", "fdr_ctx_set_replay_gemm",
                 "fdr_impala_set_replay_gemm"):
        assert diag not in names and diag in declared_functions((DIAG,))


def test_header_declares_the_boundary():
    names = declared_functions()
    for required in ("fdr_perturb", "fdr_policy_forward", "fdr_rollout", "fdr_fd_weights", "fdr_fd_grad",
                     "fdr_dsgd_step", "fdr_ctx_create", "fdr_last_error"):
        assert required in names


def test_library_exports_every_declared_symbol():
    from fdr import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    missing = [n for n in declared_functions() if not hasattr(lib, n)]
    assert not missing, missing
    assert set(_lib.EXPORTS) == set(declared_functions())


def test_version_and_workspace_queries():
    from fdr import _lib
    assert "gfx950" in _lib.version()
    assert _lib.lib.fdr_fd_grad_workspace_bytes(2048, 6092) >= 6092 * 8
    assert _lib.lib.fdr_dsgd_workspace_bytes(6092) > 0
    # the MOMENTS output length is queryable and checked (fdr 0.3; it was 2P + 3 before)
    assert _lib.version().startswith("fdr 0.5")   # 0.5: impala bn refresh, atari strategies; 0.4: done_threshold
    assert _lib.lib.fdr_fd_grad_fused_out_len(_lib.FDR_WEIGHT_ZSCORE, 6092, 4096) == 6092
    assert _lib.lib.fdr_fd_grad_fused_out_len(_lib.FDR_WEIGHT_MOMENTS, 6092, 4096) == 2 * 6092 + 1 + 4096
    assert _lib.lib.fdr_fd_grad_fused_out_len(_lib.FDR_WEIGHT_MOMENTS, 6092, 0) == -1
    assert _lib.lib.fdr_fd_grad_fused_out_len(7, 6092, 4096) == -1


def test_argument_validation_without_gpu():
    """Invalid calls are rejected before any device work (no GPU needed)."""
    from fdr import _lib
    rc = _lib.lib.fdr_perturb(None, None, 10, None, 100, None, None, 1, 0.1, None, None)
    assert rc == _lib.FDR_ERR_INVALID
    assert b"NULL" in _lib.lib.fdr_last_error()
    pd = _lib.PolicyDesc(_lib.FDR_POLICY_MUJOCO, 17, 6, 32, 6092, None, None)   # hidden != 64
    ld = _lib.LanesDesc(1, 0, None, 0, None, None, 0.0, None)
    rc = _lib.lib.fdr_policy_forward(None, ctypes.byref(pd), ctypes.byref(ld), 1, 1, 1, 1, None)
    assert rc == _lib.FDR_ERR_UNSUPPORTED


def test_ctx_create_reports_missing_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from fdr import _lib
    c = ctypes.c_void_p()
    assert _lib.lib.fdr_ctx_create(0, ctypes.byref(c)) == _lib.FDR_ERR_HIP


def _atari_calls(lib):
    """The four entry points that take an fdr_atari_desc, every other argument NULL / 0: the descriptor is checked
    first, before any pointer is looked at."""
    return {
        "fdr_atari_rollout": lambda d: lib.fdr_atari_rollout(None, d, None, 0, 0, 0, None, None, None, None, None, None,
                                                             None, 0, None),
        "fdr_atari_forward": lambda d: lib.fdr_atari_forward(None, d, None, 0, None, None, None, None, 0, None),
        "fdr_atari_bn_refresh": lambda d: lib.fdr_atari_bn_refresh(None, d, None, 0, None, 0.1, None, None, None, 0,
                                                                   None),
        "fdr_atari_strategies": lambda d: lib.fdr_atari_strategies(None, d, None, 0, 0, None, None, None, 0, None),
    }


@pytest.mark.parametrize("entry", ["fdr_atari_rollout", "fdr_atari_forward", "fdr_atari_bn_refresh",
                                   "fdr_atari_strategies"])
def test_atari_descriptor_validation_without_gpu(entry):
    """NULL desc -> INVALID, n_act outside 1..32 -> UNSUPPORTED, n_params off by one -> INVALID, in that order and with
    these texts, at every Atari entry point (no GPU needed: rejected before any device work)."""
    from fdr import _lib
    lib = _lib.lib
    call = _atari_calls(lib)[entry]
    P = lib.fdr_atari_num_params(6)
    assert P > 0
    assert call(None) == _lib.FDR_ERR_INVALID
    assert lib.fdr_last_error() == b"atari desc is NULL"
    for n_act in (0, 33):
        d = _lib.AtariDesc(n_act, 2, 3, 0, 0, P, None, None)
        assert call(ctypes.byref(d)) == _lib.FDR_ERR_UNSUPPORTED
        assert lib.fdr_last_error() == b"n_act must be in 1..32"
    for off in (-1, 1):
        d = _lib.AtariDesc(6, 2, 3, 0, 0, P + off, None, None)
        assert call(ctypes.byref(d)) == _lib.FDR_ERR_INVALID
        assert lib.fdr_last_error() == b"n_params does not match the AtariPolicy layout"


def test_atari_workspace_queries_reject_null_desc():
    from fdr import _lib
    assert _lib.lib.fdr_atari_workspace_bytes(None, 4) == -1
    assert _lib.lib.fdr_atari_strategies_workspace_bytes(None, 300, 3) == -1


def test_workspace_sizes_are_pinned():
    """The byte counts the library reported before the learner / Atari host code was split into units (read from that
    build): callers size their buffers with these queries, so a refactor of the plans must not move them."""
    from fdr import _lib
    lib = _lib.lib
    assert lib.fdr_dsgd_workspace_bytes(6092) == 4160
    assert lib.fdr_fd_grad_workspace_bytes(2048, 6092) == 1559552
    assert lib.fdr_fd_grad_fused_workspace_bytes(2048, 2, 6092, _lib.FDR_WEIGHT_ZSCORE) == 1593088
    assert lib.fdr_fd_grad_fused_workspace_bytes(2048, 2, 6092, _lib.FDR_WEIGHT_CENTERED_RANK) == 1593088
    assert lib.fdr_fd_grad_fused_workspace_bytes(2048, 2, 6092, _lib.FDR_WEIGHT_MOMENTS) == 3152640
    assert lib.fdr_fd_grad_fused_counter_bytes(2048, 6092) == 256
    assert lib.fdr_bn_refresh_workspace_bytes(16) == 11520
    P = lib.fdr_atari_num_params(6)
    d = _lib.AtariDesc(6, 2, 3, 0, 0, P, None, None)   # 4 lanes x 2 envs per lane
    assert lib.fdr_atari_workspace_bytes(ctypes.byref(d), 4) == 10962944
    # 300 lanes: past the 256-lane chunk, so the plan is the chunk's, not the call's
    assert lib.fdr_atari_strategies_workspace_bytes(ctypes.byref(d), 300, 3) == 704272384
