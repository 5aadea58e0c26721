"""Drop-in for the reference's evaluate_best_player.py (evaluate_best_player.py:20-98): the best
model's PV-MCTS player (pv_mcts.pv_mcts_action at temperature 0, on the MI355X engine with the
Python-search semantics and the fused HIP evaluator) against the random player, EP_GAME_COUNT
games alternating the first move, printing "VS_Random <average point>" for the training monitors.
The alpha-beta and plain-MCTS opponents are disabled in the reference (:87-95); the plain-MCTS one is
available here behind EP_VS_MCTS (off by default: the output is the reference's), as a batched search over
random playouts on the engine (uttt_amd.PlayoutEvaluator), and as mcts_action_factory for single moves; the
alpha-beta one behind EP_VS_ALPHABETA (off by default too), as alpha_beta_action_factory: the engine's exact
endgame solver where the position is small enough, a fallback player before that."""
import os
import random
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import uttt_cpp  # noqa: E402
import pv_mcts  # noqa: E402
from pv_mcts import pv_mcts_action  # noqa: E402
from uttt_amd import arena  # noqa: E402
from uttt_amd.selfplay import symmetry_from_env  # noqa: E402
from uttt_amd.model import DualNetwork  # noqa: E402

CPP_GAME_AVAILABLE = True
EP_GAME_COUNT = 10
EP_VS_MCTS = False  # also print "VS_MCTS <average point>" (evaluate_best_player.py:93-95, commented out there)
EP_VS_ALPHABETA = False  # also print "VS_AlphaBeta <average point>" (evaluate_best_player.py:89-91, likewise)

device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
first_player_point = arena.first_player_point


def random_action(state):
    """game.py:234-236 (Python's global `random`)."""
    legal_actions = state.legal_actions()
    return legal_actions[random.randint(0, len(legal_actions) - 1)]


def mcts_action_factory(evaluate_count=1000, playouts=64, seed=0, solve=None):
    """game.py:294-379's mcts_action on the engine: next_action(state) runs one tree of evaluate_count
    simulations whose leaves are valued by `playouts` random playouts (game.py:277-287; uniform priors, PUCT
    in place of UCB1) and returns the first legal action with the most root visits (game.py:374-379).
    solve: None, or a dict of uttt_amd.SolvedLeaves arguments (max_empties, max_nodes, priors): the leaves the
    exact solver proves then carry their game-theoretic value; next_action.evaluator is that SolvedLeaves
    (its solved / budget / skipped counts)."""
    from uttt_amd.selfplay import PlayoutEvaluator, SolvedLeaves
    search = arena.PvMcts(1, max(50, evaluate_count))
    evaluator = PlayoutEvaluator(search.engine, playouts, seed)
    if solve is not None:
        evaluator = SolvedLeaves(evaluator, search.engine, **solve)

    def mcts_action(state):
        (v,) = search.visits([state], evaluator, evaluate_count, pv_mcts.MCTS_BATCH_SIZE)
        ns = [int(x) for x in v]
        return state.legal_actions()[ns.index(max(ns))]

    mcts_action.evaluator = evaluator
    return mcts_action


def alpha_beta_action_factory(max_nodes=65536, fallback=None):
    """game.py:262-274's alpha_beta_action where it finishes: next_action(state) returns the exact solver's
    action (Engine.solve: the lowest move of the largest game-theoretic value, alpha_beta_action's choice)
    when the position is solved within max_nodes nodes per move, else fallback(state) (default:
    mcts_action_factory(), created on first use)."""
    from uttt_amd import Engine, solver
    engine = Engine(1)
    players = {"fallback": fallback}

    def alpha_beta_action(state):
        _, action, status, _, _ = engine.solve([state], max_nodes)
        if status[0] == solver.SOLVED and action[0] >= 0:
            return int(action[0])
        if players["fallback"] is None:
            players["fallback"] = mcts_action_factory()
        return players["fallback"](state)

    return alpha_beta_action


def play(next_actions):
    state = uttt_cpp.State()
    while not state.is_done():
        next_action = next_actions[0] if state.is_first_player() else next_actions[1]
        state = state.next(next_action(state))
    return first_player_point(state)


def evaluate_algorithm_of(label, next_actions):
    total_point = 0
    for i in range(EP_GAME_COUNT):
        if i % 2 == 0:
            total_point += play(next_actions)
        else:
            total_point += 1 - play(list(reversed(next_actions)))
        print("\rEvaluate {}/{}".format(i + 1, EP_GAME_COUNT), end="")
    print("")
    average_point = total_point / EP_GAME_COUNT
    print(label, average_point)
    return average_point


def evaluate_best_player():
    model = DualNetwork().to(device)
    model.load_state_dict(torch.load("./model/best.pth", map_location=device, weights_only=True))
    model.eval()
    next_pv_mcts_action = pv_mcts_action(model, 0.0)
    point = evaluate_algorithm_of("VS_Random", (next_pv_mcts_action, random_action))
    if EP_VS_MCTS:
        # UTTT_SYMMETRY = off (default) | hashed | average | 0..7, optional :seed: the model's leaves only
        print("VS_MCTS", arena.evaluate_vs_playouts(model, EP_GAME_COUNT, evaluate_count=pv_mcts.PV_EVALUATE_COUNT,
                                                    batch_size=pv_mcts.MCTS_BATCH_SIZE,
                                                    symmetry=symmetry_from_env())[0])
    if EP_VS_ALPHABETA:
        evaluate_algorithm_of("VS_AlphaBeta", (next_pv_mcts_action, alpha_beta_action_factory()))
    del model
    return point


if __name__ == "__main__":
    evaluate_best_player()
