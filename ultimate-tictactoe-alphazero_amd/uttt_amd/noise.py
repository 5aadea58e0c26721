"""Root exploration noise (csrc/uttt_noise.h): the CPU counterpart of what Engine.set_root_noise
makes the engine write into its roots, and the parsers of the two self-play settings.

  root_noise_host(states, stream, ply, epsilon, alpha, seed)   (eta, mixed priors) of roots with uniform priors
  parse_root_noise(spec)            None | (eps, alpha[, seed]) | "eps,alpha[,seed]" -> None or (eps, alpha, seed)
  parse_temperature_plies(spec)     None | n | (n, late) | "n[,late]"                -> (plies or None, late)
  root_noise_from_env() / temperature_plies_from_env()   UTTT_ROOT_NOISE / UTTT_TEMPERATURE_PLIES (unset: off)
"""
import ctypes
import os

import numpy as np

from . import _lib
from ._lib import UtttState, check, ptr


def root_noise_host(states, stream, ply, epsilon, alpha, seed=0):
    """(eta, priors), each (n, 81) f32: row r holds, at ranks below the root's number of legal moves (ascending
    action order), the Dirichlet(alpha) draw keyed by (seed, stream[r], ply[r]) and the mixed prior
    fmaf(epsilon, eta, (1 - epsilon) / L); zeros past them. In self-play stream is the global game id and ply the
    game's ply; in a plain search the tree index and 0."""
    from .engine import as_states
    st = as_states(states)
    n = len(st)
    stream = np.ascontiguousarray(np.broadcast_to(np.asarray(stream, np.int64), (n,)))
    ply = np.ascontiguousarray(np.broadcast_to(np.asarray(ply, np.int32), (n,)))
    eta = np.zeros((n, 81), np.float32)
    pri = np.zeros((n, 81), np.float32)
    check(_lib.load().uttt_root_noise_host(st.ctypes.data_as(ctypes.POINTER(UtttState)), n, ptr(stream, ctypes.c_int64),
                                           ptr(ply, ctypes.c_int32), float(epsilon), float(alpha),
                                           ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), ptr(eta, ctypes.c_float),
                                           ptr(pri, ctypes.c_float)))
    return eta, pri


def parse_root_noise(spec):
    """None / "" / "off" -> None; (eps, alpha[, seed]) or "eps,alpha[,seed]" -> (eps, alpha, seed). epsilon 0 is
    off too. The ranges are the engine's: epsilon in [0, 1], alpha in [1/32, 32]."""
    if spec is None or (isinstance(spec, str) and spec.strip().lower() in ("", "off")):
        return None
    parts = [x.strip() for x in spec.split(",")] if isinstance(spec, str) else list(spec)
    if len(parts) not in (2, 3):
        raise ValueError(f"root noise is eps,alpha[,seed] (got {spec!r})")
    try:
        eps, alpha = float(parts[0]), float(parts[1])
        seed = int(parts[2]) if len(parts) == 3 else 0
    except (TypeError, ValueError):
        raise ValueError(f"root noise is eps,alpha[,seed] (got {spec!r})") from None
    if not 0.0 <= eps <= 1.0 or not 1.0 / 32.0 <= alpha <= 32.0:
        raise ValueError(f"root noise: epsilon must be in [0, 1] and alpha in [1/32, 32] (got {spec!r})")
    return (eps, alpha, seed) if eps > 0.0 else None


def parse_temperature_plies(spec, late_temperature=0.0):
    """None / "" / "off" -> (None, late_temperature); n, (n, late) or "n[,late]" -> (n, late)."""
    if spec is None or (isinstance(spec, str) and spec.strip().lower() in ("", "off")):
        return None, float(late_temperature)
    if isinstance(spec, str):
        parts = [x.strip() for x in spec.split(",")]
    else:
        parts = list(spec) if isinstance(spec, (tuple, list)) else [spec]
    if len(parts) not in (1, 2):
        raise ValueError(f"a temperature schedule is n[,late] (got {spec!r})")
    try:
        plies = int(parts[0])
        late = float(parts[1]) if len(parts) == 2 else float(late_temperature)
    except (TypeError, ValueError):
        raise ValueError(f"a temperature schedule is n[,late] (got {spec!r})") from None
    if plies < 0 or not 0.0 <= late < float("inf"):
        raise ValueError(f"a temperature schedule needs n >= 0 and a finite late temperature >= 0 (got {spec!r})")
    return plies, late


def root_noise_from_env():
    """UTTT_ROOT_NOISE = "eps,alpha[,seed]" (unset: off), as parse_root_noise reads it."""
    return parse_root_noise(os.environ.get("UTTT_ROOT_NOISE"))


def temperature_plies_from_env():
    """UTTT_TEMPERATURE_PLIES = "n[,late]" (unset: off; late defaults to 0), as parse_temperature_plies reads it."""
    return parse_temperature_plies(os.environ.get("UTTT_TEMPERATURE_PLIES"))


__all__ = ["root_noise_host", "parse_root_noise", "parse_temperature_plies", "root_noise_from_env",
           "temperature_plies_from_env"]
