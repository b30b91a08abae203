"""The one way a native library of `build.LIBS` is loaded. Fails loudly: a missing library, or one
built from other sources than the tree's, is an error, never a fallback.

torch is imported first so that the library's libamdhip64.so.7 dependency binds to the HIP
runtime torch already loaded (one runtime per process: device pointers from the torch caching
allocator and streams from torch.cuda are then valid inside the library).
"""

from __future__ import annotations

import ctypes
import os

from . import build


def build_info(L, prefix: str) -> dict:
    """<prefix>_build_info() as a dict (src = source hash the library was compiled from)."""
    return dict(kv.split("=", 1) for kv in getattr(L, prefix + "_build_info")().decode().split() if "=" in kv)


def load(name: str, path: str, error: type, prefix: str, declare, no_fallback: str):
    """Library `name` of build.LIBS from `path`, with `declare(L)` applied for the argtypes of its
    `prefix`_* functions. Raises `error`; `no_fallback` ends the message for a missing file."""
    import torch  # noqa: F401  (bind the HIP runtime torch ships, see module docstring)

    if not os.path.exists(path):
        raise error(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`"
            f" ({no_fallback})")
    L = ctypes.CDLL(path)
    declare(L)
    getattr(L, prefix + "_last_error").restype = ctypes.c_char_p
    getattr(L, prefix + "_build_info").restype = ctypes.c_char_p
    info = build_info(L, prefix)
    if os.environ.get("NMMO_ALLOW_STALE") != "1" and os.path.isdir(build.CSRC):
        want = build.source_hash(name)
        if info.get("src") != want:
            raise error(
                f"{path} was built from other sources (src={info.get('src')}, tree={want}): "
                "rebuild it (`python -m nmmo_amd.build --force`)")
    return L
