"""Loader for the in-tree native modules.

* ``_runtime``  -- the C++ parameter-server runtime (engine, consistency models, control
  plane, checkpoint I/O); CPU only, always required.
* ``_kernels``  -- the gfx950 HIP kernels (torch extension). Required whenever a GPU tensor
  reaches an op: on a GPU box a missing or stale build raises instead of silently falling
  back to eager PyTorch.
* ``_evalk``    -- the held-out evaluation kernels (binned-AUC histograms, fused eval head): a second,
  small torch extension with the same rule -- a GPU tensor without it raises.
* ``_optk``     -- the global-norm gradient-clipping kernels of the dense clock (fp64 partial sums of
  squares, the clipping Adam): a third small torch extension, same rule.
"""
from __future__ import annotations

import importlib
import os

_kernels = None
_kernels_err: Exception | None = None
_evalk = None
_evalk_err: Exception | None = None
_optk = None
_optk_err: Exception | None = None
_runtime = None
_runtime_err: Exception | None = None


def kernels():
    """Return the HIP kernel module or raise a loud error."""
    global _kernels, _kernels_err
    if _kernels is None and _kernels_err is None:
        try:
            import torch  # noqa: F401  (libtorch must be loaded first)

            _kernels = importlib.import_module("minips_amd._kernels")
        except Exception as e:  # pragma: no cover - depends on the build
            _kernels_err = e
    if _kernels is None:
        raise RuntimeError(
            "minips_amd._kernels (gfx950 HIP kernels) is not built or failed to load: "
            f"{_kernels_err!r}. Run `python tools/build.py` (or __graft_entry__.build())."
        )
    return _kernels


def evalk():
    """Return the HIP evaluation-kernel module or raise a loud error."""
    global _evalk, _evalk_err
    if _evalk is None and _evalk_err is None:
        try:
            import torch  # noqa: F401  (libtorch must be loaded first)

            _evalk = importlib.import_module("minips_amd._evalk")
        except Exception as e:  # pragma: no cover - depends on the build
            _evalk_err = e
    if _evalk is None:
        raise RuntimeError(
            "minips_amd._evalk (gfx950 HIP evaluation kernels) is not built or failed to load: "
            f"{_evalk_err!r}. Run `python tools/build.py` (or __graft_entry__.build())."
        )
    return _evalk


def optk():
    """Return the HIP gradient-clipping kernel module or raise a loud error."""
    global _optk, _optk_err
    if _optk is None and _optk_err is None:
        try:
            import torch  # noqa: F401  (libtorch must be loaded first)

            _optk = importlib.import_module("minips_amd._optk")
        except Exception as e:  # pragma: no cover - depends on the build
            _optk_err = e
    if _optk is None:
        raise RuntimeError(
            "minips_amd._optk (gfx950 HIP gradient-clipping kernels) is not built or failed to load: "
            f"{_optk_err!r}. Run `python tools/build.py` (or __graft_entry__.build())."
        )
    return _optk


def runtime():
    """Return the C++ runtime module or raise."""
    global _runtime, _runtime_err
    if _runtime is None and _runtime_err is None:
        try:
            _runtime = importlib.import_module("minips_amd._runtime")
        except Exception as e:  # pragma: no cover
            _runtime_err = e
    if _runtime is None:
        raise RuntimeError(
            f"minips_amd._runtime (C++ PS runtime) is not built: {_runtime_err!r}. Run `python tools/build.py`."
        )
    return _runtime


def kernels_available() -> bool:
    try:
        kernels()
        return True
    except RuntimeError:
        return False


def evalk_available() -> bool:
    try:
        evalk()
        return True
    except RuntimeError:
        return False


def optk_available() -> bool:
    try:
        optk()
        return True
    except RuntimeError:
        return False


def native_dir() -> str:
    return os.path.dirname(os.path.abspath(__file__))
