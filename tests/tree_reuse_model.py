"""TEST INFRASTRUCTURE ONLY — a small Python restatement of the C++-semantics search (csrc/engine/select.h, DESIGN.md
§3) with append semantics, on the engine's own flat node layout, plus tree reuse: re-root at the
played move, merge the duplicate child sets, top the root up to S visits.

The rules and the hash evaluator come from oracle.core. Everything the search computes is float32, operation by
operation: PUCT = q + (P * sqrtf(total)) / (1 + n) with q = -W / n, strict '>' from -1e9 in child order, a flush of
k = min(B, S - done) identical copies appending k child blocks, the sequential prior sum, and the back-up adding the
value k times with the sign flipping upward. With reuse off it is oracle.core.pv_mcts_scores_hash bit for bit
(test_tree_reuse_host.py anchors that).

A tree is a list of nodes [W, P, N, action, L, first, k] in pool order: the root at 0, its block at 1..L, every
expansion appended. `as_array` gives it as uttt_amd.reuse.TREE_DTYPE.
"""
import numpy as np

from oracle import core

F = np.float32
NO_ACTION = 0x7F
W, P, N, ACT, LL, FIRST, K = range(7)


def hash_evaluator(state):
    pol, val = core.hash_eval(state.tensor_nchw())
    return pol, F(val)


class Tree:
    def __init__(self, state, evaluator=hash_evaluator):
        self.state = state
        self.evaluator = evaluator
        self.done = 0      # TreeCtl.sims_done
        self.evals = 0     # leaves sent to the evaluator
        legal = state.legal_actions()
        L = len(legal)
        up = F(1.0) / F(L) if L else F(0.0)
        self.nodes = [[F(0.0), F(0.0), 0, NO_ACTION, L, 1 if L else 0, 1 if L else 0]]
        self.nodes += [[F(0.0), up, 0, a, 0, 0, 0] for a in legal]

    # ---------------------------------------------------------------- search --
    def search(self, S, B):
        """Run until the root has S visits (select_wave + expand_backup, one tree)."""
        nd = self.nodes
        while self.done < S:
            s, node, path = self.state, 0, [0]
            while True:
                r = nd[node]
                cnt = r[K] * r[LL]
                if cnt == 0:
                    break
                total = r[N] - (0 if node == 0 else r[K])
                sq = np.sqrt(F(total), dtype=F)
                best, bi = F(-1e9), None
                for c in range(cnt):
                    ch = nd[r[FIRST] + c]
                    cn = ch[N]
                    q = -ch[W] / F(cn) if cn > 0 else F(0.0)
                    u = (ch[P] * sq) / F(1 + cn)
                    v = q + u
                    if v > best:
                        best, bi = v, c
                assert bi is not None
                node = r[FIRST] + bi
                path.append(node)
                s = s.next(nd[node][ACT])
            depth = len(path) - 1
            legal = s.legal_actions()
            if s.is_lose() or not legal:
                v = F(1.0) if s.is_lose() else F(-0.0)
                for d, pn in enumerate(path):
                    nd[pn][W] = nd[pn][W] + (-v if (depth - d) & 1 else v)
                    nd[pn][N] += 1
                self.done += 1
                continue
            k = min(B, S - self.done)
            pol, val = self.evaluator(s)
            self.evals += 1
            pri = [F(pol[a]) for a in legal]
            tot = F(0.0)
            for x in pri:
                tot = tot + x
            un = F(1.0) / F(len(legal))
            pri = [x / tot if tot > 0 else un for x in pri]
            nb = len(nd)
            for _ in range(k):
                nd += [[F(0.0), p, 0, a, 0, 0, 0] for p, a in zip(pri, legal)]
            for d, pn in enumerate(path):
                x = -val if (depth - d) & 1 else val
                w = nd[pn][W]
                for _ in range(k):
                    w = w + x
                nd[pn][W] = w
                nd[pn][N] += k
            nd[node][LL], nd[node][FIRST], nd[node][K] = len(legal), nb, k
            self.done += k
        return self

    # --------------------------------------------------------------- results --
    def legal(self):
        return [self.nodes[1 + i][ACT] for i in range(self.nodes[0][LL])]

    def visits(self):
        return np.array([self.nodes[1 + i][N] for i in range(self.nodes[0][LL])], np.int32)

    def priors(self):
        return np.array([self.nodes[1 + i][P] for i in range(self.nodes[0][LL])], F)

    def set_priors(self, p):
        for i, x in enumerate(p):
            self.nodes[1 + i][P] = F(x)

    def scores(self, temperature):
        v = self.visits().astype(F)
        if temperature == 0:
            out = np.zeros(len(v), F)
            if len(v):
                out[int(np.argmax(v))] = 1.0
            return out
        return core.boltzman(v, temperature)

    def as_array(self):
        from uttt_amd.reuse import TREE_DTYPE
        out = np.zeros(len(self.nodes), TREE_DTYPE)
        for i, r in enumerate(self.nodes):
            out[i] = (r[W], r[P], r[N], r[ACT], r[LL], r[FIRST], r[K])
        return out

    # --------------------------------------------------------------- re-root --
    def reroot(self, action):
        """The tree of the position after `action`, built by recursion where the engine and its
        host mirror run a breadth-first queue: the layout is assigned afterwards, level by level."""
        nd = self.nodes
        root = nd[0]
        ci = next(root[FIRST] + i for i in range(root[LL]) if nd[root[FIRST] + i][ACT] == action)
        c = nd[ci]
        out = Tree.__new__(Tree)
        out.evaluator, out.evals = self.evaluator, 0
        out.state = self.state.next(action)
        if c[K] == 0 or c[LL] == 0:  # never expanded, or terminal: a fresh root
            fresh = Tree(out.state, self.evaluator)
            out.nodes, out.done = fresh.nodes, 0
            return out
        kc, Lp = c[K], c[LL]
        # a node of the new tree: (record, [source child blocks as (first, count)])
        new = [[c[W], F(0.0), c[N] - kc, NO_ACTION, Lp, 1, 1]]
        pending = []  # per queued node, the blocks of `nd` that become its children, in order
        for r in range(Lp):
            dups = [nd[c[FIRST] + i * Lp + r] for i in range(kc)]
            w = dups[0][W]
            for d in dups[1:]:
                w = w + d[W]
            new.append([w, dups[0][P], sum(d[N] for d in dups), dups[0][ACT], max(d[LL] for d in dups), 0,
                        sum(d[K] for d in dups)])
            pending.append([(d[FIRST], d[K] * d[LL]) for d in dups if d[K] * d[LL]])
        q = 1
        while q < len(new):
            blocks = pending[q - 1]
            if blocks:
                new[q][FIRST] = len(new)
                for first, cnt in blocks:
                    for j in range(cnt):
                        ch = nd[first + j]
                        new.append([ch[W], ch[P], ch[N], ch[ACT], ch[LL], 0, ch[K]])
                        pending.append([(ch[FIRST], ch[K] * ch[LL])] if ch[K] * ch[LL] else [])
            q += 1
        out.nodes = new
        out.done = c[N] - kc
        # what select_wave relies on: a node's visits less its own k are its children's
        for r in new[1:]:
            if r[K] * r[LL]:
                assert r[N] - r[K] == sum(new[r[FIRST] + j][N] for j in range(r[K] * r[LL]))
        assert new[0][N] == sum(x[N] for x in new[1:1 + Lp])
        return out


def noisy_priors(tree, game, ply, noise):
    """k_root_noise on the model's root: fmaf(eps, eta, (1 - eps) * P), with eta from uttt_amd.noise.root_noise_host."""
    from fractions import Fraction

    from uttt_amd import noise as un
    import wide_deep
    eps, alpha, seed = noise
    eta, _ = un.root_noise_host(wide_deep.pack_states([tree.state]), [game], [ply], eps, alpha, seed=seed)
    out = []
    for e, p in zip(eta[0], tree.priors()):
        c = F(F(1.0) - F(eps)) * p
        out.append(f32_nearest(Fraction(float(F(eps))) * Fraction(float(e)) + Fraction(float(c))))
    return out


def f32_nearest(x):
    """The f32 nearest the Fraction x (ties to even): fmaf's one rounding, in exact arithmetic."""
    from fractions import Fraction
    if x == 0:
        return F(0.0)
    y = F(float(x))  # within one f32 ulp of x; the exact comparison below picks among the neighbours
    cands = sorted({float(np.nextafter(y, F(-np.inf))), float(y), float(np.nextafter(y, F(np.inf)))})
    best = min(cands, key=lambda c: (abs(Fraction(c) - x), int(np.float32(c).view(np.uint32)) & 1))
    return F(best)


def play_game(seed, S, B, temperature=1.0, reuse=False, noise=None, game=0, max_plies=81, trace=None):
    """self_play_cpp.play with RandomState(seed) and the hash evaluator, on the model. Returns actions, f64
    policies (81 wide), values, the leaves evaluated and the largest node count seen."""
    mt = core.MT(seed)
    s = core.OrState.initial()
    tree = None
    acts, pols, evals, max_nodes = [], [], 0, 0
    ply = 0
    while not s.is_done() and ply < max_plies:
        tree = tree.reroot(acts[-1]) if (reuse and tree is not None) else Tree(s)
        if noise is not None:
            tree.set_priors(noisy_priors(tree, game, ply, noise))
        carried = tree.done
        tree.search(S, B)
        evals += tree.evals
        max_nodes = max(max_nodes, len(tree.nodes))
        if trace is not None:
            trace.append((carried, tree.evals, len(tree.nodes)))
        legal = s.legal_actions()
        assert legal == tree.legal() and int(tree.visits().sum()) == S
        pol, idx = core.policy_and_sample(mt, tree.scores(temperature))
        row = np.zeros(81, np.float64)
        row[legal] = pol
        pols.append(row)
        acts.append(legal[idx])
        s = s.next(legal[idx])
        ply += 1
    v = -1 if s.is_lose() else 0
    values = np.array([v if (i & 1) == 0 else -v for i in range(len(acts))], np.int64)
    return {"actions": np.array(acts, np.int64), "policies": np.array(pols), "values": values, "evals": evals,
            "max_nodes": max_nodes}
