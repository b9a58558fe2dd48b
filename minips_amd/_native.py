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
* ``_ftrlk``    -- the FTRL-Proximal apply of sparse table rows (``SparseTable(optimizer="ftrl")``): a
  fourth small torch extension, same rule.
* ``_wdftrlk``  -- the split-row apply with two rules, row-wise Adagrad on the deep columns and FTRL-Proximal
  on the wide ones (``SparseTable(split=..., wide_optimizer="ftrl")``): a fifth small torch extension, same
  rule.
* ``_fmk``      -- the factorization-machine forward and backward over a CSR batch of pulled rows
  (``ops.fm_forward`` / ``ops.fm_backward``): a sixth small torch extension, same rule.
* ``_dfmk``     -- DeepFM's FM interaction term over the assembled Wide & Deep input (``ops.wd_fm_forward`` /
  ``ops.wd_fm_backward``): a seventh small torch extension, same rule.
* ``_dcnk``     -- the Deep & Cross layers over the assembled Wide & Deep input (``ops.wd_cross_forward`` /
  ``ops.wd_cross_backward`` / ``ops.wd_cross_fold``): an eighth small torch extension, same rule.
* ``_ffmk``     -- the field-aware factorization-machine forward and backward over a CSR batch of pulled rows
  (``ops.ffm_forward`` / ``ops.ffm_backward``): a ninth small torch extension, same rule.
* ``_gbdtk``    -- the fixed-point histogram GBDT kernels (``ops.gbdt_bin`` / ``gbdt_grad`` / ``gbdt_hist`` /
  ``gbdt_split`` / ``gbdt_leaf`` / ``gbdt_advance`` / ``gbdt_predict``): a tenth small torch extension, same rule.
* ``_ldak``     -- the fixed-point LDA collapsed Gibbs kernels (``ops.lda_sample`` / ``lda_delta`` /
  ``lda_loglik``): an eleventh small torch extension, same rule.
* ``_w2vk``     -- the word2vec skip-gram negative-sampling kernels (``ops.sgns_lookups`` / ``sgns_forward`` /
  ``sgns_backward``): a twelfth small torch extension, same rule.
"""
from __future__ import annotations

import importlib
import os

_loaded: dict = {}  # module name -> the module, or the exception its import raised


def _load(name: str, what: str, torch_ext: bool = True):
    """minips_amd.<name>, imported once; a missing or stale build raises a loud error on every call."""
    if name not in _loaded:
        try:
            if torch_ext:
                import torch  # noqa: F401  (libtorch must be loaded first)

            _loaded[name] = importlib.import_module("minips_amd." + name)
        except Exception as e:  # pragma: no cover - depends on the build
            _loaded[name] = e
    mod = _loaded[name]
    if isinstance(mod, Exception):
        state, fix = ("is not built or failed to load", " (or __graft_entry__.build()).") if torch_ext else \
            ("is not built", ".")
        raise RuntimeError(f"minips_amd.{name} ({what}) {state}: {mod!r}. Run `python tools/build.py`{fix}")
    return mod


def _available(loader) -> bool:
    try:
        loader()
        return True
    except RuntimeError:
        return False


def kernels():
    """Return the HIP kernel module or raise a loud error."""
    return _load("_kernels", "gfx950 HIP kernels")


def evalk():
    """Return the HIP evaluation-kernel module or raise a loud error."""
    return _load("_evalk", "gfx950 HIP evaluation kernels")


def optk():
    """Return the HIP gradient-clipping kernel module or raise a loud error."""
    return _load("_optk", "gfx950 HIP gradient-clipping kernels")


def ftrlk():
    """Return the HIP FTRL-Proximal kernel module or raise a loud error."""
    return _load("_ftrlk", "gfx950 HIP FTRL-Proximal kernel")


def wdftrlk():
    """Return the HIP Adagrad + FTRL-Proximal split-row kernel module or raise a loud error."""
    return _load("_wdftrlk", "gfx950 HIP Adagrad + FTRL-Proximal split-row kernel")


def fmk():
    """Return the HIP factorization-machine kernel module or raise a loud error."""
    return _load("_fmk", "gfx950 HIP factorization-machine kernels")


def dfmk():
    """Return the HIP DeepFM interaction-term kernel module or raise a loud error."""
    return _load("_dfmk", "gfx950 HIP DeepFM interaction-term kernels")


def dcnk():
    """Return the HIP Deep & Cross kernel module or raise a loud error."""
    return _load("_dcnk", "gfx950 HIP Deep & Cross kernels")


def ffmk():
    """Return the HIP field-aware factorization-machine kernel module or raise a loud error."""
    return _load("_ffmk", "gfx950 HIP field-aware factorization-machine kernels")


def gbdtk():
    """Return the HIP histogram GBDT kernel module or raise a loud error."""
    return _load("_gbdtk", "gfx950 HIP histogram GBDT kernels")


def ldak():
    """Return the HIP LDA Gibbs kernel module or raise a loud error."""
    return _load("_ldak", "gfx950 HIP LDA Gibbs kernels")


def w2vk():
    """Return the HIP word2vec (skip-gram, negative sampling) kernel module or raise a loud error."""
    return _load("_w2vk", "gfx950 HIP word2vec skip-gram negative-sampling kernels")


def runtime():
    """Return the C++ runtime module or raise."""
    return _load("_runtime", "C++ PS runtime", torch_ext=False)


def kernels_available() -> bool:
    return _available(kernels)


def evalk_available() -> bool:
    return _available(evalk)


def optk_available() -> bool:
    return _available(optk)


def ftrlk_available() -> bool:
    return _available(ftrlk)


def wdftrlk_available() -> bool:
    return _available(wdftrlk)


def fmk_available() -> bool:
    return _available(fmk)


def dfmk_available() -> bool:
    return _available(dfmk)


def dcnk_available() -> bool:
    return _available(dcnk)


def ffmk_available() -> bool:
    return _available(ffmk)


def gbdtk_available() -> bool:
    return _available(gbdtk)


def ldak_available() -> bool:
    return _available(ldak)


def w2vk_available() -> bool:
    return _available(w2vk)


def native_dir() -> str:
    return os.path.dirname(os.path.abspath(__file__))
