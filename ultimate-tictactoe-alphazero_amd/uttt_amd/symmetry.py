"""The eight symmetries of the square on Ultimate Tic-Tac-Toe positions (csrc/uttt_sym.h).

Symmetry g = r + 4 f (r quarter turns, f a mirror first) is, on the (9, 9) image, np.rot90(np.fliplr(img) if f else
img, k=r). It takes action a to ACTION_PERM[g, a] and the flat image position R * 9 + C to IMAGE_PERM[g, R * 9 + C].
A position and its image have the same value; an evaluator's policy row p' for the image is the row
p[a] = p'[ACTION_PERM[g, a]] for the position. The tables come from the engine library's C functions (the rules
layer the kernels compile too), so Python, host and device share one definition.

  transform_states(states, sym)   packed states -> their images (uttt_states_transform_host)
  hashed_symmetry(states, seed)   the position-keyed choice SymmetricLeaves("hashed") makes
  transform_inputs(x, sym)        NCHW (n, 3, 9, 9) inputs -> the images' inputs (an index gather)
  transform_policy(p, sym)        (n, 81) policies of positions -> the policies of their images
  policy_from_image(p, sym)       (n, 81) rows evaluated on the images -> rows of the positions
  augment_history(history, sym)   [[x (9,9,3), policy (81,), value], ...] -> the eight images of each sample
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import STATE_DTYPE, UtttState, check, ptr

COUNT = 8


def _tables():
    lib = _lib.load()
    perm = np.zeros((COUNT, 81), np.int32)
    for g in range(COUNT):
        check(lib.uttt_sym_action_perm(g, ptr(perm[g], ctypes.c_int32)))
    inverse = np.array([lib.uttt_sym_inverse(g) for g in range(COUNT)], np.int64)
    compose = np.array([[lib.uttt_sym_compose(g, h) for h in range(COUNT)] for g in range(COUNT)], np.int64)
    # image position R * 9 + C <-> action (uttt_game.cpp:256-257): rows and columns are 3 * board + cell coordinates
    pos = np.arange(81)
    R, C = pos // 9, pos % 9
    action_at = (R // 3 * 3 + C // 3) * 9 + (R % 3) * 3 + C % 3
    image_index = np.argsort(action_at)
    image = image_index[perm[:, action_at]]  # position -> action -> its image -> that action's position
    return perm.astype(np.int64), image.astype(np.int64), inverse, compose


ACTION_PERM, IMAGE_PERM, INVERSE, COMPOSE = _tables()
# the gathers: the image's entry at d comes from the position's entry at *_SRC[g, d]
ACTION_SRC = np.argsort(ACTION_PERM, axis=1)
IMAGE_SRC = np.argsort(IMAGE_PERM, axis=1)


def compose(g, h):
    """The symmetry that applies h, then g."""
    return int(COMPOSE[g, h])


def inverse(g):
    return int(INVERSE[g])


def _sym_array(sym, n):
    s = np.array(np.broadcast_to(np.asarray(sym, np.int64), (n,)))  # a writable copy (torch.from_numpy)
    if n and (s.min() < 0 or s.max() >= COUNT):
        raise ValueError("a symmetry must be 0..7")
    return s


def transform_states(states, sym):
    """T_sym[i] of each packed state (STATE_DTYPE array); sym an int or one per state."""
    st = np.ascontiguousarray(states, STATE_DTYPE)
    s8 = _sym_array(sym, len(st)).astype(np.int8)
    out = np.zeros(len(st), STATE_DTYPE)
    check(_lib.load().uttt_states_transform_host(st.ctypes.data_as(ctypes.POINTER(UtttState)), len(st),
                                                 ptr(s8, ctypes.c_int8),
                                                 out.ctypes.data_as(ctypes.POINTER(UtttState))))
    return out


def hashed_symmetry(states, seed=0):
    """The hashed choice per state (int8): a function of the position's 243 network-input bits and the seed."""
    st = np.ascontiguousarray(states, STATE_DTYPE)
    out = np.zeros(len(st), np.int8)
    check(_lib.load().uttt_states_symmetry_host(st.ctypes.data_as(ctypes.POINTER(UtttState)), len(st),
                                                ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF),
                                                ptr(out, ctypes.c_int8)))
    return out


def _gather_last(a, table, sym):
    """a[i, ..., table[sym[i], j]] over the last axis, for a numpy array or a torch tensor."""
    if isinstance(a, np.ndarray):
        idx = table[_sym_array(sym, len(a))]
        idx = idx.reshape((len(a),) + (1,) * (a.ndim - 2) + (idx.shape[1],))
        return np.take_along_axis(a, np.broadcast_to(idx, a.shape), axis=-1)
    import torch
    if torch.is_tensor(sym):
        s = sym.to(device=a.device, dtype=torch.long)
    else:
        s = torch.from_numpy(_sym_array(sym, len(a))).to(a.device)
    idx = torch.from_numpy(table).to(a.device)[s]
    idx = idx.reshape((len(a),) + (1,) * (a.dim() - 2) + (idx.shape[1],))
    return torch.gather(a, a.dim() - 1, idx.expand(a.shape))


def transform_inputs(x, sym, out=None):
    """NCHW (n, 3, 9, 9) inputs of positions -> the inputs of their images: per sample and plane
    np.rot90(np.fliplr(img) if f else img, r). numpy or torch; sym an int, an array or a tensor; out (torch): the
    tensor to write into, distinct from x."""
    n = len(x)
    flat = x.reshape(n, 3, 81)
    if out is not None:
        import torch
        s = sym.to(device=x.device, dtype=torch.long) if torch.is_tensor(sym) else \
            torch.from_numpy(_sym_array(sym, n)).to(x.device)
        idx = torch.from_numpy(IMAGE_SRC).to(x.device)[s].reshape(n, 1, 81).expand(n, 3, 81)
        torch.gather(flat, 2, idx, out=out.view(n, 3, 81))
        return out
    return _gather_last(flat, IMAGE_SRC, sym).reshape(x.shape)


def transform_policy(p, sym, out=None):
    """(n, 81) policies of positions -> the policies of their images: out[i, ACTION_PERM[g, a]] = p[i, a]."""
    if out is not None:
        import torch
        s = sym.to(device=p.device, dtype=torch.long) if torch.is_tensor(sym) else \
            torch.from_numpy(_sym_array(sym, len(p))).to(p.device)
        torch.gather(p, 1, torch.from_numpy(ACTION_SRC).to(p.device)[s], out=out)
        return out
    return _gather_last(p, ACTION_SRC, sym)


def policy_from_image(p, sym):
    """(n, 81) rows an evaluator gave for the images -> the rows of the positions: out[i, a] = p[i, ACTION_PERM[g, a]]
    (the policy back-mapping; what k_sym_rows computes)."""
    return _gather_last(p, ACTION_PERM, sym)


def augment_history(history, sym=None):
    """[[x (9, 9, 3), policy (81,), value], ...] -> the images of each sample under `sym` (default: all eight, so
    8 N samples, sample i's images at 8 i .. 8 i + 7 in symmetry order), dtypes kept, values unchanged."""
    syms = list(range(COUNT)) if sym is None else [int(s) for s in np.atleast_1d(sym)]
    out = []
    for x, pol, val in history:
        x = np.asarray(x)
        pol_a = np.asarray(pol)
        for g in syms:
            f, r = divmod(g, 4)
            img = np.rot90(np.flip(x, axis=1) if f else x, k=r, axes=(0, 1))
            out.append([np.ascontiguousarray(img), pol_a[ACTION_SRC[g]], val])
    return out


__all__ = ["ACTION_PERM", "ACTION_SRC", "COMPOSE", "COUNT", "IMAGE_PERM", "IMAGE_SRC", "INVERSE", "augment_history",
           "compose", "hashed_symmetry", "inverse", "policy_from_image", "transform_inputs", "transform_policy",
           "transform_states"]
