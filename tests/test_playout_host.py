"""CPU tests of the random-playout evaluator's host side (uttt_playout_host, csrc/uttt_playout.h): it equals
an independent pure-Python restatement of game.py:277-287 with the counter-based draw (Python-int mix64, the
key from the NCHW input bits, the oracle's rules), its sign convention on hand-built terminal and one-move
positions, the canonical key (a function of stones and legal moves, not of `active`), argument checks."""
import ctypes
import random

import numpy as np
import pytest

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15


def mix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def key_of(ostate, seed):
    """hash_words(the four words of the 243 NCHW input bits) ^ mix64(seed)."""
    x = ostate.tensor_nchw()
    h = GOLD
    for i in range(4):
        w = 0
        for j in range(64 * i, min(64 * i + 64, 243)):
            if x[j] != 0:
                w |= 1 << (j - 64 * i)
        h = mix64(h ^ w)
    return h ^ mix64(seed)


def playout_py(s, h, j):
    sign, ply = 1, 0
    while True:
        if s.is_lose():
            return -sign
        legal = s.legal_actions()
        if not legal:
            return 0
        r = mix64(h + ((j * 128 + ply + 1) * GOLD))
        idx = (((r >> 32) * len(legal)) >> 32) & 0xFFFFFFFF
        s = s.next(legal[idx])
        sign, ply = -sign, ply + 1


def pack(ostates):
    from uttt_amd._lib import STATE_DTYPE
    arr = np.zeros(len(ostates), STATE_DTYPE)
    for i, s in enumerate(ostates):
        p, e, mp, me, a = s.arrays()
        for x in range(81):
            arr["own"][i, x // 27] |= int(p.reshape(81)[x]) << (x % 27)
            arr["opp"][i, x // 27] |= int(e.reshape(81)[x]) << (x % 27)
        arr["mains"][i] = sum(int(mp[b]) << b for b in range(9)) | sum(int(me[b]) << (16 + b) for b in range(9))
        arr["active"][i] = a
    return arr


def host_counts(lib, states, playouts, seed):
    from uttt_amd._lib import UtttState
    states = np.ascontiguousarray(states)
    wins = np.full(len(states), -7, np.int32)
    losses = np.full(len(states), -7, np.int32)
    rc = lib.uttt_playout_host(states.ctypes.data_as(ctypes.POINTER(UtttState)), len(states), playouts, seed,
                               wins.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                               losses.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    return rc, wins, losses


def free_move_position(core, active):
    """The side to move has won board 0 and is sent there (or anywhere): a free move into 69 empty cells."""
    p = np.zeros((9, 9), np.int32)
    e = np.zeros((9, 9), np.int32)
    p[0, [0, 1, 2]] = 1
    e[4, 0] = e[5, 0] = e[8, 0] = 1
    return core.OrState.from_arrays(p, e, [1] + [0] * 8, [0] * 9, active)


def position_set(core):
    """~40 positions along random lines, the initial position (81 legal moves) and free moves into more than
    64 empty cells."""
    rng = random.Random(11)
    out = [core.OrState.initial(), free_move_position(core, 0), free_move_position(core, -1)]
    while len(out) < 40:
        s = core.OrState.initial()
        while not s.is_done() and len(out) < 40:
            if rng.random() < 0.25:
                out.append(s)
            s = s.next(rng.choice(s.legal_actions()))
    return out


def test_host_playouts_equal_python_restatement(engine_lib, oracle_lib):
    ostates = position_set(oracle_lib)
    assert len(ostates[0].legal_actions()) == 81
    assert len(ostates[1].legal_actions()) == 69 and len(ostates[2].legal_actions()) == 69
    packed = pack(ostates)
    seed = 0x1234567890ABCDEF
    # playout j is a function of (key, j) alone: one restated result per (position, j), summed per P
    res = np.array([[playout_py(s, key_of(s, seed), j) for j in range(65)] for s in ostates])
    assert set(np.unique(res)) <= {-1, 0, 1} and (res > 0).any() and (res < 0).any()
    for P in (1, 64, 65):
        rc, wins, losses = host_counts(engine_lib, packed, P, seed)
        assert rc == 0
        assert np.array_equal(wins, (res[:, :P] > 0).sum(axis=1)), P
        assert np.array_equal(losses, (res[:, :P] < 0).sum(axis=1)), P
    # another seed gives other games (the seed enters the key)
    rc, wins2, _ = host_counts(engine_lib, packed, 64, seed + 1)
    rc, wins1, _ = host_counts(engine_lib, packed, 64, seed)
    assert rc == 0 and not np.array_equal(wins1, wins2)


def _from_arrays(lib, p, e, mp, me, active):
    from uttt_amd._lib import STATE_DTYPE, UtttState
    st = np.zeros(1, STATE_DTYPE)
    i32 = ctypes.POINTER(ctypes.c_int32)
    arrs = [np.ascontiguousarray(np.asarray(a, np.int32).reshape(-1)) for a in (p, e, mp, me)]
    assert lib.uttt_state_from_arrays(*(a.ctypes.data_as(i32) for a in arrs), active,
                                      st.ctypes.data_as(ctypes.POINTER(UtttState))) == 0
    return st


def test_sign_convention(engine_lib):
    z = np.zeros((9, 9), np.int32)
    # the only legal move (board 2, cell 2) wins board 2 and with it the main board's top row
    p, e = z.copy(), z.copy()
    p[2, [0, 1, 5, 7]] = 1
    e[2, [3, 4, 6, 8]] = 1
    win_in_one = _from_arrays(engine_lib, p, e, [1, 1, 0, 0, 0, 0, 0, 0, 0], [0] * 9, 2)
    from uttt_amd._lib import UtttState
    assert engine_lib.uttt_state_is_done(win_in_one.ctypes.data_as(ctypes.POINTER(UtttState))) == 0
    lost = _from_arrays(engine_lib, z, z, [0] * 9, [1, 0, 0, 0, 1, 0, 0, 0, 1], -1)
    drawn = _from_arrays(engine_lib, z, z, [1, 0, 1, 1, 0, 0, 0, 1, 1], [0, 1, 0, 0, 1, 1, 1, 0, 0], -1)
    for P in (1, 64, 65, 4096):
        rc, wins, losses = host_counts(engine_lib, np.concatenate([win_in_one, lost, drawn]), P, 5)
        assert rc == 0
        assert wins.tolist() == [P, 0, 0] and losses.tolist() == [0, P, 0], P


def test_key_is_canonical_in_active(engine_lib):
    """Only board 6 is open: active == -1 and active == 6 have the same stones and legal moves, hence the same
    key and the same playouts; a different open position does not."""
    z = np.zeros((9, 9), np.int32)
    p, e = z.copy(), z.copy()
    p[6, [0, 4]] = 1
    e[6, [1, 8]] = 1
    mp = [1, 0, 1, 1, 0, 0, 0, 1, 1]
    me = [0, 1, 0, 0, 1, 1, 0, 0, 0]
    a = _from_arrays(engine_lib, p, e, mp, me, -1)
    b = _from_arrays(engine_lib, p, e, mp, me, 6)
    e2 = e.copy()
    e2[6, 8], e2[6, 7] = 0, 1
    c = _from_arrays(engine_lib, p, e2, mp, me, 6)
    rc, wins, losses = host_counts(engine_lib, np.concatenate([a, b, c]), 256, 9)
    assert rc == 0
    assert wins[0] == wins[1] and losses[0] == losses[1]
    assert 0 < wins[0] + losses[0] <= 256
    assert (wins[2], losses[2]) != (wins[0], losses[0])


@pytest.mark.parametrize("P", [0, 4097, -1])
def test_playout_count_is_checked(engine_lib, P):
    from uttt_amd import initial_states
    rc, wins, _ = host_counts(engine_lib, initial_states(1), P, 0)
    assert rc == -1  # UTTT_ERR_ARG
    assert b"4096" in engine_lib.uttt_last_error()
    assert wins[0] == -7
