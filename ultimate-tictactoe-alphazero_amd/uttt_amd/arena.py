"""Batched arena evaluation on the Python PV-MCTS semantics.

The reference's evaluate_network.py plays EN_GAME_COUNT games one after
another, each move a pv_mcts.py search (Python objects, one network call per
flush of <= 8 leaves). Here all games advance together: per move, the games
whose side to move plays model m form one batched search on engine m
(UTTT_SEMANTICS_PY: root evaluated by the first flush, expand replaces,
PUCT as NumPy 2 evaluates pv_mcts.py:120-130), and each round evaluates one
leaf per game in a single network call.

Game g draws its moves from RandomState(seed_base + g), so its record equals
the reference's play() after np.random.seed(seed_base + g) (same players).
"""
import numpy as np

from .engine import as_states
from .selfplay import BatchedSearch, NetworkEvaluator, PlayoutEvaluator, SolvedLeaves


def scores_from_visits(visits, temperature):
    """pv_mcts.py:175-181 on the root children's visit counts: one-hot first maximum
    (temperature 0, float64 array) or boltzman in Python floats (:190-192, a list;
    raises ZeroDivisionError like the reference when no child was visited)."""
    ns = [int(x) for x in visits]
    if temperature == 0:
        s = np.zeros(len(ns))
        s[int(np.argmax(ns))] = 1
        return s
    xs = [x ** (1 / temperature) for x in ns]
    return [x / sum(xs) for x in xs]


def first_player_point(state):
    """evaluate_network.py:26-30."""
    if state.is_lose():
        return 0 if state.is_first_player() else 1
    return 0.5


def _engine_state(state):
    import uttt_cpp
    if isinstance(state, uttt_cpp.State):
        return state
    return uttt_cpp.State(state.pieces, state.enemy_pieces, state.main_board_pieces, state.main_board_enemy_pieces,
                          state.active_board)


class PvMcts:
    """pv_mcts.py:133-181 for many root states at once (one tree each)."""

    def __init__(self, max_trees, max_sims=50, device=None):
        self.search = BatchedSearch(max_trees, max_sims, device)
        self.engine = self.search.engine

    def visits(self, states, evaluator, evaluate_count=50, batch_size=8):
        """states: uttt_cpp.State / game.State objects or a packed STATE_DTYPE array
        -> list of root-children visit counts (int arrays, legal-action order)."""
        roots = as_states(states) if isinstance(states, np.ndarray) else as_states([_engine_state(s) for s in states])
        self.search.run(roots, evaluator, evaluate_count, batch_size, semantics="py")
        v, L = self.search.visits()
        return [v[i, :L[i]].copy() for i in range(len(roots))]

    def scores(self, states, evaluator, temperature, evaluate_count=50, batch_size=8):
        return [scores_from_visits(v, temperature) for v in self.visits(states, evaluator, evaluate_count, batch_size)]


class ModelEvaluator:
    """A DualNetwork-shaped model (model(x) -> policies (N,81), values (N,1)) as an engine
    evaluator; inputs are moved to the model's device (models may live on the CPU)."""

    def __init__(self, model):
        import torch
        self.model = model.eval()
        self.dev = next((p.device for p in model.parameters()), None)
        self.torch = torch

    def __call__(self, x, n):
        with self.torch.no_grad():
            xi = x[:n] if self.dev is None else x[:n].to(self.dev)
            p, v = self.model(xi)
        return p.to(x.device).float(), v.to(x.device).float().reshape(n, -1)


def model_evaluator(model, max_batch=None, engine=None, kind=None, symmetry=None):
    """Engine evaluator for a model: the fused HIP evaluator for a DualNetwork (given the engine;
    nnfast.evaluator_kind), else NetworkEvaluator when the model lives on the GPU (no copies),
    ModelEvaluator otherwise. symmetry (selfplay.parse_symmetry's forms; default off; needs the engine): the
    evaluator wrapped in SymmetricLeaves."""
    from .selfplay import parse_symmetry, with_symmetry
    if parse_symmetry(symmetry) is not None and engine is None:
        raise ValueError("model_evaluator: symmetry needs the engine whose leaves are transformed")
    if engine is not None:
        from .nnfast import FusedNetworkEvaluator, evaluator_kind
        if evaluator_kind(model, kind) == "fused":
            return with_symmetry(FusedNetworkEvaluator(model, engine), engine, symmetry)
    dev = next((p.device for p in model.parameters()), None)
    if dev is not None and dev.type == "cuda" and max_batch:
        model.eval()
        return with_symmetry(NetworkEvaluator(model, max_batch), engine, symmetry)
    return with_symmetry(ModelEvaluator(model), engine, symmetry)


def _play_games(searches, evaluators, evaluate_counts, game_count, temperature, seed_base, batch_size, progress):
    """evaluate_network.py:58-104's games, all concurrent: player m (searches[m], evaluators[m],
    evaluate_counts[m] simulations per move) moves first in game g when g % 2 == m. Game g draws from
    RandomState(seed_base + g). Returns (player 0's average point, per-game first-player points, per-game
    action lists)."""
    import uttt_cpp
    states = [uttt_cpp.State() for _ in range(game_count)]
    rngs = [np.random.RandomState(seed_base + g) for g in range(game_count)]
    order = [(0, 1) if g % 2 == 0 else (1, 0) for g in range(game_count)]  # (first player, second player)
    actions = [[] for _ in range(game_count)]
    while True:
        live = [g for g in range(game_count) if not states[g].is_done()]
        if not live:
            break
        groups = [[g for g in live if order[g][0 if states[g].is_first_player() else 1] == m] for m in (0, 1)]
        for m, idx in enumerate(groups):  # one move per live game per iteration
            if not idx:
                continue
            vis = searches[m].visits([states[g] for g in idx], evaluators[m], evaluate_counts[m], batch_size)
            for g, v in zip(idx, vis):
                legal = states[g].legal_actions()
                sc = scores_from_visits(v, temperature)
                if len(sc) != len(legal):
                    raise ValueError(f"Score size mismatch: scores={len(sc)}, legal_actions={len(legal)}")
                a = int(rngs[g].choice(legal, p=sc))
                actions[g].append(a)
                states[g] = states[g].next(a)
        if progress:
            progress(game_count - len(live), game_count)
    points = [first_player_point(s) for s in states]
    total = sum(p if g % 2 == 0 else 1 - p for g, p in enumerate(points))
    return total / game_count, points, actions


def evaluate_network(model0, model1, game_count=50, temperature=1.0, seed_base=0, evaluate_count=50,
                     batch_size=8, device=None, make_evaluator=None, progress=None, symmetry=None):
    """evaluate_network.py:58-104 with all games concurrent. Game g: model0 moves first when g is
    even, model1 when odd (:78-82). Returns (model0's average point, per-game first-player points,
    per-game action lists). make_evaluator(model, engine) -> engine evaluator (default: the model
    called on the engine's input batch; e.g. nnfast.FusedNetworkEvaluator for a DualNetwork). symmetry: the
    default evaluators' SymmetricLeaves setting (model_evaluator; default off)."""
    searches = [PvMcts(game_count, evaluate_count, device) for _ in range(2)]
    if make_evaluator is None:
        evaluators = (model_evaluator(model0, game_count, searches[0].engine, symmetry=symmetry),
                      model_evaluator(model1, game_count, searches[1].engine, symmetry=symmetry))
    else:
        evaluators = (make_evaluator(model0, searches[0].engine), make_evaluator(model1, searches[1].engine))
    return _play_games(searches, evaluators, (evaluate_count, evaluate_count), game_count, temperature, seed_base,
                       batch_size, progress)


def evaluate_vs_playouts(model, game_count=10, playouts=64, opponent_evaluate_count=1000, seed_base=0,
                         temperature=0.0, evaluate_count=50, batch_size=8, device=None, make_evaluator=None,
                         playout_seed=0, progress=None, opponent_solve=None, symmetry=None):
    """The model's PV-MCTS player against plain MCTS over random playouts (the reference's commented-out
    VS_MCTS opponent, evaluate_best_player.py:93-95 with game.py:294-379's mcts_action: there UCB1 over one
    playout per evaluation, here the same search as the model's with PlayoutEvaluator in place of the network:
    uniform priors, the mean of `playouts` playouts as the value, opponent_evaluate_count simulations per
    move). All games run concurrently as in evaluate_network, on the Python-search semantics; the model moves
    first in even games. Returns (the model's average point, per-game first-player points, per-game action
    lists). make_evaluator(model, engine) -> the model's engine evaluator (default as evaluate_network).
    opponent_solve: None, or a dict of SolvedLeaves arguments (max_empties, max_nodes, priors): the opponent
    then plays with an exact endgame, and the result has a fourth entry, its leaf counts over all games
    (SolvedLeaves.counts: {"skipped", "solved", "budget"})."""
    searches = [PvMcts(game_count, evaluate_count, device), PvMcts(game_count, opponent_evaluate_count, device)]
    if make_evaluator is None:
        ev = model_evaluator(model, game_count, searches[0].engine, symmetry=symmetry)
    else:
        ev = make_evaluator(model, searches[0].engine)
    opponent = PlayoutEvaluator(searches[1].engine, playouts, playout_seed)
    if opponent_solve is not None:
        opponent = SolvedLeaves(opponent, searches[1].engine, **opponent_solve)
    result = _play_games(searches, (ev, opponent), (evaluate_count, opponent_evaluate_count), game_count, temperature,
                         seed_base, batch_size, progress)
    if opponent_solve is not None:
        return result + (opponent.counts(),)
    return result


def evaluate_network_match(model0, model1, games=1024, opening_plies=4, evaluate_count=50, batch_size=8, sample_plies=0,
                           seed=0, device=None, make_evaluator=None, symmetry=None, progress=None):
    """evaluate_network's question asked of a device-resident match (match.play_match): model0 against model1
    over `games` games from games // 2 random openings of opening_plies plies, each played with both colours,
    the moves the most visited ones (sample_plies > 0: the first plies sampled from the visit counts). Returns a
    match.MatchResult: model0's score, the Elo difference and its 95% interval from the pair scores.
    make_evaluator(model, engine) -> engine evaluator (default: model_evaluator, with `symmetry`)."""
    from . import match
    if games < 2 or games % 2:
        raise ValueError(f"evaluate_network_match: games must be even and at least 2 (got {games})")

    def factory(model):
        if make_evaluator is not None:
            return lambda engine: make_evaluator(model, engine)
        return lambda engine: model_evaluator(model, engine.max_trees, engine, symmetry=symmetry)

    openings = match.random_openings(games // 2, opening_plies, seed)
    return match.play_match(match.Player(factory(model0), evaluate_count, batch_size),
                            match.Player(factory(model1), evaluate_count, batch_size), games, openings, paired=True,
                            sample_plies=sample_plies, seed=seed, device=device, progress=progress)


def first_player_value(state):
    """self_play.py:20-25."""
    if state.is_lose():
        return -1 if state.is_first_player() else 1
    return 0


def self_play_py(model, game_count, seed_base=0, temperature=1.0, evaluate_count=50, batch_size=8, device=None,
                 make_evaluator=None, progress=None, symmetry=None, temperature_plies=None, late_temperature=0.0):
    """self_play.py:66-99 (the Python self-play: pv_mcts.py searches) for game_count games at once.
    Game g draws from RandomState(seed_base + g) (= play(model) after np.random.seed(seed_base + g)).
    Returns one history per game: [input (9,9,3) float64, policies (81 Python floats, 0 for
    illegal actions), value (first_player_value at ply 0, then alternating)]. temperature_plies (default off):
    moves from that ply on use late_temperature."""
    import uttt_cpp
    search = PvMcts(game_count, evaluate_count, device)
    ev = make_evaluator(model, search.engine) if make_evaluator else \
        model_evaluator(model, game_count, search.engine, symmetry=symmetry)
    states = [uttt_cpp.State() for _ in range(game_count)]
    rngs = [np.random.RandomState(seed_base + g) for g in range(game_count)]
    hist = [[] for _ in range(game_count)]
    while True:
        live = [g for g in range(game_count) if not states[g].is_done()]
        if not live:
            break
        vis = search.visits([states[g] for g in live], ev, evaluate_count, batch_size)
        for g, v in zip(live, vis):
            st = states[g]
            legal = st.legal_actions()
            late = temperature_plies is not None and len(hist[g]) >= temperature_plies
            scores = scores_from_visits(v, late_temperature if late else temperature)
            policies = [0] * 81
            for action, policy in zip(legal, scores):
                policies[action] = policy
            x = np.asarray(st.to_input_tensor(), dtype=np.float64).reshape(9, 9, 3)
            hist[g].append([x, policies, None])
            states[g] = st.next(int(rngs[g].choice(legal, p=scores)))
        if progress:
            progress(game_count - len(live), game_count)
    for g in range(game_count):
        value = first_player_value(states[g])
        for rec in hist[g]:
            rec[2] = value
            value = -value
    return hist


__all__ = ["ModelEvaluator", "first_player_value", "self_play_py", "PvMcts", "evaluate_network", "first_player_point", "model_evaluator",
           "scores_from_visits", "evaluate_vs_playouts", "evaluate_network_match"]
