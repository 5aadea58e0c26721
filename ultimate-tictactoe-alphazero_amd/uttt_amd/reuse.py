"""Tree reuse (csrc/uttt_reroot.h, csrc/engine/reroot.h): the node records Engine.tree returns, and
the CPU counterpart of what Engine.reroot and a reusing self-play move make of a tree.

  TREE_DTYPE                    one node: W, P (f32), N, action, L, first, k (the fields of the 16-byte record)
  unpack(raw) / pack(tree)      (n, 4) uint32 records <-> TREE_DTYPE array (py-semantics flag bits are dropped)
  reroot_host(tree, state, a)   the tree re-rooted at action a, in the canonical breadth-first layout
  tree_reuse_from_env()         UTTT_TREE_REUSE (unset or 0: off)
"""
import ctypes
import os

import numpy as np

from . import _lib
from ._lib import UtttState, check, ptr

TREE_DTYPE = np.dtype([("W", "<f4"), ("P", "<f4"), ("N", "<i4"), ("action", "<i4"), ("L", "<i4"), ("first", "<i4"),
                       ("k", "<i4")])
NO_ACTION = 0x7F


def unpack(raw):
    """(n, 4) uint32 node records -> TREE_DTYPE array. W and P keep their bits."""
    raw = np.ascontiguousarray(raw, np.uint32).reshape(-1, 4)
    out = np.zeros(len(raw), TREE_DTYPE)
    out["W"] = raw[:, 0].view(np.float32)
    out["P"] = raw[:, 1].view(np.float32)
    out["N"] = raw[:, 2] & 0xFFFF
    out["action"] = (raw[:, 2] >> 16) & 0x7F
    out["L"] = (raw[:, 2] >> 23) & 0x7F
    out["first"] = raw[:, 3] & 0xFFFFF
    out["k"] = raw[:, 3] >> 20
    return out


def pack(tree):
    """TREE_DTYPE array -> (n, 4) uint32 node records."""
    tree = np.asarray(tree, TREE_DTYPE)
    raw = np.zeros((len(tree), 4), np.uint32)
    raw[:, 0] = np.ascontiguousarray(tree["W"]).view(np.uint32)
    raw[:, 1] = np.ascontiguousarray(tree["P"]).view(np.uint32)
    raw[:, 2] = (tree["N"].astype(np.uint32) & 0xFFFF) | ((tree["action"].astype(np.uint32) & 0x7F) << 16) | \
        ((tree["L"].astype(np.uint32) & 0x7F) << 23)
    raw[:, 3] = (tree["first"].astype(np.uint32) & 0xFFFFF) | (tree["k"].astype(np.uint32) << 20)
    return raw


def reroot_host(tree, state, action):
    """The tree (TREE_DTYPE array or (n, 4) uint32 records) of a "cpp" search from `state`, re-rooted at `action`
    (uttt_reroot_host): the played child's subtree with its duplicate child sets merged, or a fresh root when
    that child has no children, as a TREE_DTYPE array in the layout the device writes. ValueError for an action
    that is not a move of the root."""
    from .engine import as_states
    raw = pack(tree) if getattr(tree, "dtype", None) == TREE_DTYPE else np.ascontiguousarray(tree, np.uint32).reshape(-1, 4)
    st = as_states([state] if not isinstance(state, np.ndarray) else state.reshape(-1)[:1])
    out = np.zeros((max(len(raw), 82), 4), np.uint32)
    n = ctypes.c_int32()
    check(_lib.load().uttt_reroot_host(ptr(raw, ctypes.c_uint32), len(raw), st.ctypes.data_as(ctypes.POINTER(UtttState)),
                                       int(action), ptr(out, ctypes.c_uint32), ctypes.byref(n)))
    return unpack(out[:n.value])


def tree_reuse_from_env():
    """UTTT_TREE_REUSE=1 switches tree reuse on (unset, empty or 0: off)."""
    return os.environ.get("UTTT_TREE_REUSE", "").strip().lower() not in ("", "0", "off", "false")


__all__ = ["TREE_DTYPE", "NO_ACTION", "unpack", "pack", "reroot_host", "tree_reuse_from_env"]
