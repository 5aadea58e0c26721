/*
 * uttt_engine.h — C ABI of the MI355X-native Ultimate Tic-Tac-Toe self-play engine.
 *
 * This is the drop-in boundary for the reference's native hot path
 * (cpp/uttt_game.h, cpp/uttt_mcts.h behind the pybind11 module `uttt_cpp`,
 * cpp/python_bindings.cpp:49-107). Plain C types only: pointers, sizes,
 * status codes. Every function returns UTTT_OK (0) or a negative UTTT_ERR_*;
 * uttt_last_error() gives the message of the calling thread's last failure.
 *
 * Two layers:
 *   1. Rules on one host-side state value (what `uttt_cpp.State` binds).
 *   2. The engine: thousands of PUCT trees in SoA arrays in HBM, advanced in
 *      lock-step rounds by HIP kernels (gfx950). A round = every unfinished
 *      tree descends to its next unevaluated leaf (absorbing terminal
 *      simulations), the leaves are handed to an evaluator as one NCHW batch,
 *      and the results are expanded + backed up. Self-play adds the per-move
 *      policy target, numpy-exact move sampling and game records on device.
 *
 * Semantics are those of cpp/uttt_mcts.cpp:84-196 bit for bit (see DESIGN.md,
 * "Exact semantics"); the only structural change is that the k identical
 * copies of a flushed leaf (uttt_mcts.cpp:121-135 queues the same leaf k times
 * because there is no virtual loss) are evaluated once and replayed k times.
 */
#ifndef UTTT_ENGINE_H
#define UTTT_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UTTT_OK 0
#define UTTT_ERR_ARG (-1)      /* invalid argument                                  */
#define UTTT_ERR_HIP (-2)      /* HIP runtime error                                 */
#define UTTT_ERR_CAPACITY (-3) /* node pool / path / record arena exhausted         */
#define UTTT_ERR_ORDER (-4)    /* call out of sequence (e.g. apply before select)   */
#define UTTT_ERR_NODEVICE (-5) /* no gfx950 device / device ordinal out of range    */
#define UTTT_ERR_NONFINITE (-6) /* evaluator returned NaN/Inf (legal prior or value) */

#define UTTT_ACTIONS 81
#define UTTT_MAX_SIMS 4095 /* most simulations per search (uttt_engine_create max_sims): the 16-byte node
                               record keeps N in 16 bits, k in 12, the first child in 20 */
#define UTTT_INPUT_SIZE 243 /* (3, 9, 9) NCHW f32 per position */

/* Packed, side-to-move-relative position (32 bytes; same bits on host and device).
 * own[w]/opp[w]: small boards 3w..3w+2, board b's 9 cells at bits 9*(b%3)..+8,
 *   so bit (a % 27) of word (a / 27) is action a = board*9 + cell.
 * mains: bits 0..8 main_board_pieces, bits 16..24 main_board_enemy_pieces.
 * active: -1 (any board) or 0..8.
 * Replaces UTTT::State's int arrays (cpp/uttt_game.h:49-54). */
typedef struct uttt_state {
    uint32_t own[3];
    uint32_t opp[3];
    uint32_t mains;
    int32_t active;
} uttt_state_t;

const char *uttt_last_error(void);
const char *uttt_version(void);

/* ---------------------------------------------------------------- rules --- */
/* State() — cpp/uttt_game.cpp:9-21 */
void uttt_state_initial(uttt_state_t *out);
/* State(pieces, enemy_pieces, main, main_enemy, active) — cpp/uttt_game.cpp:24-32.
 * Arrays are [board][cell] row-major. Values must be 0/1 and active in -1..8
 * (the reference does not validate; out-of-range input is UB there). */
int uttt_state_from_arrays(const int32_t pieces[81], const int32_t enemy_pieces[81],
                           const int32_t main_board_pieces[9], const int32_t main_board_enemy_pieces[9],
                           int32_t active_board, uttt_state_t *out);
/* get_pieces/... — cpp/uttt_game.h:42-46 */
void uttt_state_to_arrays(const uttt_state_t *s, int32_t pieces[81], int32_t enemy_pieces[81],
                          int32_t main_board_pieces[9], int32_t main_board_enemy_pieces[9],
                          int32_t *active_board);
/* State::next — cpp/uttt_game.cpp:97-145 (any action 0..80, unvalidated as in the reference) */
int uttt_state_next(const uttt_state_t *s, int32_t action, uttt_state_t *out);
/* State::legal_actions — cpp/uttt_game.cpp:148-191; returns the count, ascending actions in out */
int uttt_state_legal_actions(const uttt_state_t *s, int32_t out[81]);
/* is_lose / is_draw / is_done / is_first_player — cpp/uttt_game.cpp:77-94 (return 0/1) */
int uttt_state_is_lose(const uttt_state_t *s);
int uttt_state_is_draw(const uttt_state_t *s);
int uttt_state_is_done(const uttt_state_t *s);
int uttt_state_is_first_player(const uttt_state_t *s);
/* to_input_tensor — cpp/uttt_game.cpp:244-280 (HWC (9,9,3) flat) */
void uttt_state_input_hwc(const uttt_state_t *s, float out[243]);
/* The same for n states (out: n x 243 floats), e.g. the rank-0 .history build after a gather. */
int uttt_states_input_hwc(const uttt_state_t *s, int64_t n, float *out);
/* to_string — cpp/uttt_game.cpp:194-241; returns length, or -(needed) if cap too small */
int uttt_state_to_string(const uttt_state_t *s, char *buf, int32_t cap);
/* boltzman — cpp/uttt_mcts.cpp:199-216 */
int uttt_boltzman(const float *xs, int32_t n, float temperature, float *out);
/* playout — game.py:277-287, for n states, `playouts` (1..4096) uniformly random games from each: wins and
 * losses of the state's side to move (a lost state: every playout a loss; a drawn one: neither). Python's
 * `random` is replaced by a counter-based draw keyed by the position's 243 network-input bits and `seed`
 * (csrc/uttt_playout.h), so playout j is a function of (position, seed, j). Pure CPU: what uttt_playouts and
 * uttt_eval_playout_dev compute on the device, bit for bit. */
int uttt_playout_host(const uttt_state_t *states, int64_t n, int32_t playouts, uint64_t seed, int32_t *wins,
                      int32_t *losses);
/* alpha_beta / alpha_beta_action — game.py:240-274, for n late positions: the exact value of each position for
 * its side to move and of each of its legal moves. One full-depth fail-hard negamax (values -1 / 0 / +1,
 * window (-1, +1), moves ascending) per legal action a, on the child next(s, a); each of these searches
 * counts the nodes it visits and stops unsolved at max_nodes (1..2^22) (csrc/uttt_solve.h).
 *   action_values[i*81 + a]: minus the child's value; UTTT_SOLVE_UNKNOWN for an unsolved child and for an
 *     illegal action.
 *   status[i]: UTTT_SOLVE_SOLVED when some solved move wins (value +1, action the lowest such move; other
 *     moves may be unknown) or every move is solved (value the largest action value, action the lowest move
 *     that reaches it: alpha_beta_action's choice); UTTT_SOLVE_BUDGET otherwise (value 0, action -1).
 *     A terminal position is SOLVED with value -1 (lost) or 0 (drawn), action -1, nodes 0. A position that
 *     is not terminal and has more than 32 empty cells in open small boards is not searched:
 *     UTTT_SOLVE_TOO_LARGE, value 0, action -1, nodes 0.
 *   nodes[i]: nodes visited over all of the position's moves.
 * value, action, status: int8[n]; nodes: int64[n]; action_values: int8[n*81]; any of them may be NULL.
 * Pure CPU: what uttt_solve computes on the device, bit for bit. */
#define UTTT_SOLVE_SOLVED 1
#define UTTT_SOLVE_BUDGET 2
#define UTTT_SOLVE_TOO_LARGE 3
#define UTTT_SOLVE_UNKNOWN (-128)
#define UTTT_SOLVE_MAX_EMPTY 32
int uttt_solve_host(const uttt_state_t *states, int64_t n, int32_t max_nodes, int8_t *value, int8_t *action,
                    int8_t *status, int64_t *nodes, int8_t *action_values);
/* Exact endgame values laid over evaluator rows (csrc/uttt_solve.h). For position i and its
 * caller-filled row (policy + i * policy_ld: 81 f32 by action; value[i * value_ld]):
 *   more than max_empties (0..UTTT_SOLVE_MAX_EMPTY) empty cells in open small boards: UTTT_OVERLAY_SKIPPED,
 *     nothing searched, the row untouched;
 *   otherwise the position is solved as uttt_solve_host solves it, with max_nodes (1..2^22) per legal move.
 *     Not SOLVED: UTTT_SOLVE_BUDGET, the row untouched. SOLVED: UTTT_SOLVE_SOLVED and value = (float)v; with
 *     UTTT_PRIORS_OPTIMAL the policy becomes 1.0f on every legal action whose known value equals v and 0.0f on
 *     the other entries (a position won early marks its known winning moves only, a lost one every move; a
 *     terminal position keeps its policy), which the apply's legal mask and renormalisation make 1 / count.
 *     UTTT_PRIORS_KEEP leaves the policy as it is.
 * status: int8[n], may be NULL. policy_ld >= 81. Pure CPU: what uttt_eval_solve_dev computes on the device,
 * bit for bit. */
#define UTTT_OVERLAY_SKIPPED 0
#define UTTT_PRIORS_KEEP 0
#define UTTT_PRIORS_OPTIMAL 1
int uttt_solve_overlay_host(const uttt_state_t *states, int64_t n, int32_t max_empties, int32_t max_nodes,
                            int32_t priors, float *policy, int64_t policy_ld, float *value, int64_t value_ld,
                            int8_t *status);
/* The eight symmetries of the square (csrc/uttt_sym.h). g = r + 4 f, r in 0..3 quarter turns,
 * f in 0..1 a mirror first: on the (9, 9) image np.rot90(np.fliplr(img) if f else img, k = r). beta_g is the
 * same operation on a 3x3 index 3 R + C, and action a = 9 b + c goes to pi_g(a) = 9 beta_g(b) + beta_g(c).
 * T_g moves bit a of own / opp to bit pi_g(a), bit b of each half of mains to bit beta_g(b), and the active
 * board to beta_g(active) (-1 stays). An evaluator's policy row p' for T_g(s) is the row p[a] = p'[pi_g(a)]
 * for s; the value is the same. */
#define UTTT_SYM_COUNT 8
/* out[a] = pi_g(a) */
int uttt_sym_action_perm(int32_t g, int32_t out[81]);
/* The symmetry k with T_k = T_g T_h (h first, pi_k = pi_g o pi_h), and the one with T_k T_g = identity;
 * UTTT_ERR_ARG (negative) for a symmetry outside 0..7. */
int uttt_sym_compose(int32_t g, int32_t h);
int uttt_sym_inverse(int32_t g);
/* out[i] = T_{sym[i]}(states[i]); out may be states. */
int uttt_states_transform_host(const uttt_state_t *states, int64_t n, const int8_t *sym, uttt_state_t *out);
/* The hashed choice: sym[i] = the top three bits of the playout key (csrc/uttt_playout.h) of state i's 243
 * network-input bits and `seed`: a function of the stones, the legal moves and the seed alone. */
int uttt_states_symmetry_host(const uttt_state_t *states, int64_t n, uint64_t seed, int8_t *sym);
/* Dirichlet noise on root priors (csrc/uttt_noise.h): for n roots whose priors are uniform, with
 * L legal moves each, eta ~ Dirichlet(alpha) over the moves in ascending action order and the mixed priors
 * fmaf(epsilon, eta, (1 - epsilon) / L): row r, rank i at [r * 81 + i], entries at ranks >= L left untouched;
 * either output may be NULL. Row r is a function of (seed, stream[r], ply[r], L) alone: what
 * uttt_engine_set_root_noise makes the engine write, where stream is the global game id and ply the game's ply
 * in self-play, and the tree index and 0 in a plain search. Pure CPU. UTTT_ERR_ARG for epsilon outside [0, 1]
 * or alpha outside [1/32, 32]. */
int uttt_root_noise_host(const uttt_state_t *states, int64_t n, const int64_t *stream, const int32_t *ply,
                         float epsilon, float alpha, uint64_t seed, float *eta, float *priors);

/* --------------------------------------------------------------- engine --- */
typedef struct uttt_engine uttt_engine_t;

/* device: HIP ordinal (-1 = the calling thread's current device). max_trees: concurrent trees / game slots. max_sims: the
 * largest evaluate_count this engine will run, 1..4095 (sizes the node pool to the
 * exact worst case 82 + 81*max_sims nodes per tree, so it cannot overflow; the 16-byte node
 * record holds visits and child-block counts up to 4095). */
int uttt_engine_create(int32_t device, int32_t max_trees, int32_t max_sims, uttt_engine_t **out);
int uttt_engine_destroy(uttt_engine_t *eng);
/* Launch everything on `stream` (a hipStream_t, e.g. torch's current stream;
 * NULL = the null stream). Until called, the engine uses a stream of its own. */
int uttt_engine_set_stream(uttt_engine_t *eng, void *stream);
/* The engine's own non-blocking stream (created with the engine; each engine's
 * stream gets its own hardware queue when few streams exist), e.g. to run an
 * evaluator on it so that several engines on one GPU overlap. */
int uttt_engine_own_stream(uttt_engine_t *eng, void **stream);
/* Device bytes held by the engine. */
int64_t uttt_engine_device_bytes(const uttt_engine_t *eng);

/* Search semantics for uttt_search_begin_mode:
 *  UTTT_SEMANTICS_CPP  cpp/uttt_mcts.cpp (pv_mcts_cpp / self_play_cpp): root
 *                      pre-expanded uniform, expand appends k blocks, f32 PUCT;
 *  UTTT_SEMANTICS_PY   pv_mcts.py (evaluate_network / evaluate_best_player):
 *                      root evaluated by the first flush, expand replaces,
 *                      PUCT as NumPy 2 evaluates the Python expression
 *                      (float32 with sqrt in double; float64 where the
 *                      all-zero-prior fallback made the priors float64). */
#define UTTT_SEMANTICS_CPP 0
#define UTTT_SEMANTICS_PY 1
/* Start a search of n_trees independent trees (pv_mcts_scores,
 * uttt_mcts.cpp:92-103: root expanded with uniform priors 1/|legal|).
 * roots: host array of n_trees states. */
int uttt_search_begin(uttt_engine_t *eng, const uttt_state_t *roots, int32_t n_trees, int32_t evaluate_count,
                      int32_t batch_size);
/* The same with explicit semantics (replaces pv_mcts.py:133-181 when PY). */
int uttt_search_begin_mode(uttt_engine_t *eng, const uttt_state_t *roots, int32_t n_trees, int32_t evaluate_count,
                           int32_t batch_size, int32_t semantics);

/* One round of descents (uttt_mcts.cpp:109-127). Writes the pending leaves'
 * network inputs, NCHW (n,3,9,9) f32, to device memory nn_input (room for
 * max_trees*243 floats; may be NULL) in deterministic tree order, and stores
 * the number of pending leaves in *n_pending (0 = search finished). Blocks on
 * the stream to read the count. */
int uttt_search_select(uttt_engine_t *eng, float *nn_input, int32_t *n_pending);

/* The same round without reading the count on the host: launches the descents and the
 * pending-leaf scan and returns at once. The count stays on the device (uttt_search_count_ptr:
 * [0] pending leaves, [1] trees stopped by the select budget); uttt_nn_stem, the *_dev network
 * entry points and uttt_search_apply (device results, one row per leaf) read it there, so a
 * round is enqueued with no host synchronisation. A round whose count is 0 changes nothing:
 * the caller enqueues rounds until a count it copied back (uttt_search_count_copy) reads
 * [2] == 0: no tree has simulations left once this round is applied (the next select would
 * report 0). Replaces the per-round blocking read of uttt_search_select for the self-play
 * driver. */
int uttt_search_select_async(uttt_engine_t *eng);
/* Enqueue a copy of the round's counts to dst[0..2] (host, pinned for an asynchronous copy):
 * [0] pending leaves, [1] trees stopped by the select budget, [2] trees with simulations left
 * after this round's apply. */
int uttt_search_count_copy(uttt_engine_t *eng, int32_t *dst);
/* Device address of the round's counts. */
int uttt_search_count_ptr(uttt_engine_t *eng, const int32_t **count);
/* uttt_search_select_async whose scan also stores the three counts into slot ring_slot (0..7) of
 * the engine's host-visible count ring (fine-grained pinned memory, system-scope stores), with no copy
 * on the stream, and then `tag` into word 3 of the slot (a system-scope release store): the host reads
 * the counts once it has polled the tag there, no event needed (round 5, SelfPlay's network rounds). */
int uttt_search_select_async_tag(uttt_engine_t *eng, int32_t ring_slot, int32_t tag);
/* The count ring: *ring = n_slots x {pending, stopped, left after apply, tag} int32, host memory. */
int uttt_search_count_ring(uttt_engine_t *eng, const int32_t **ring, int32_t *n_slots);

/* Host copies of the pending leaves (slot order) and their multiplicity k
 * (the number of identical copies the reference would have queued). */
int uttt_search_pending(uttt_engine_t *eng, uttt_state_t *states, int32_t *copies);
/* One-tree searches (the drop-in uttt_cpp.pv_mcts_scores, python_bindings.cpp:83-100 / uttt_mcts.cpp:109-167)
 * without a copy operation or a stream synchronisation per flush (round 5): select_host launches the
 * select and the scan, which stores the counts, the pending leaf's state and its copies k into fine-grained
 * pinned host memory and then a tag the host spins on; apply_host copies the leaf's evaluation (81 priors
 * by action, value; one row or one per copy) into pinned host memory that k_apply reads directly, and
 * returns without waiting. Same results as uttt_search_select + uttt_search_pending + uttt_search_apply. */
int uttt_search_select_host(uttt_engine_t *eng, uttt_state_t *leaf, int32_t *copies, int32_t *n_pending);
int uttt_search_apply_host(uttt_engine_t *eng, const float *policy, int64_t policy_stride, const float *value,
                           int32_t rows);  /* rows: 1 (one result for the leaf's k copies) or k (one per copy,
                                              applied in order: the reference's call pattern) */

/* A one-tree search as ONE resident wave (round 6; replaces the reference's pv_mcts_scores loop,
 * uttt_mcts.cpp:84-196, as python_bindings.cpp:11-47 drives it, for uttt_cpp.pv_mcts_scores): search1_begin
 * launches the wave (root expansion included), which descends to the first flush's leaf and hands it over
 * through fine-grained pinned memory; search1_next waits for it (n_pending 1: *leaf and its copies k) or for
 * the search's end (n_pending 0; the tree's error status is raised here); search1_apply writes the leaf's
 * evaluation (one row for the k copies, or k rows in order) and a command the wave polls, and returns
 * without waiting; search1_scores copies the root's scores (pv_mcts_scores' return value: one-hot at
 * temperature 0, else boltzman, as uttt_search_scores) the wave stored at the end. No launch, copy or
 * stream synchronisation per flush; a wave left without a command for 100 ms exits and search1_next
 * resumes it. Same results as uttt_search_begin + uttt_search_select_host / apply_host + scores. */
int uttt_search1_begin(uttt_engine_t *eng, const uttt_state_t *root, int32_t sims, int32_t batch, int32_t semantics,
                       float temperature);
int uttt_search1_next(uttt_engine_t *eng, uttt_state_t *leaf, int32_t *copies, int32_t *n_pending);
int uttt_search1_apply(uttt_engine_t *eng, const float *policy, int64_t policy_stride, const float *value,
                       int32_t rows);
int uttt_search1_scores(uttt_engine_t *eng, float *scores, int32_t *n_legal);
/* Diagnostics (no reference counterpart): the resident wave's own time split up to its last hand-over, in
 * 10 ns ticks since its launch: [0] descents, [1] applies, [2] waits for the host's commands. */
int uttt_search1_time_split(uttt_engine_t *eng, int32_t *ticks3);

/* Evaluator results for the pending leaves (uttt_mcts.cpp:138-167: legal-mask,
 * sequential f32 renormalisation, expand k times, back up k times).
 * Row r of policy (>= 81 f32, stride policy_ld) / value (stride value_ld)
 * belongs to pending slot r. per_copy != 0: the rows are per queued copy
 * (slot 0's k copies first, then slot 1's ...), as the reference's model()
 * batch is. on_device: pointers are device (else host, copied on the stream). */
int uttt_search_apply(uttt_engine_t *eng, const float *policy, int64_t policy_ld, const float *value,
                      int64_t value_ld, int32_t per_copy, int32_t on_device);

/* Deterministic hash evaluator on device (test / micro-benchmark evaluator;
 * DESIGN.md "Hash evaluator"): n rows of nn_input -> policy (n,81), value (n). */
int uttt_eval_hash(uttt_engine_t *eng, const float *nn_input, int32_t n, float *policy, float *value);
/* The same evaluator on the round's pending leaves read from their states, the count read on the
 * device (after uttt_search_select_async): rows [0, count) of policy (81 f32 each) and value. */
int uttt_eval_hash_dev(uttt_engine_t *eng, float *policy, float *value);
/* The random-playout evaluator on the round's pending leaves (the count read on the device, as
 * uttt_eval_hash_dev; after uttt_search_select or uttt_search_select_async): value[row] = (wins - losses) /
 * playouts of the leaf's side to move over `playouts` (1..4096) playouts (uttt_playout_host), policy row =
 * 81 x 1.0f, which the apply's legal mask and renormalisation make 1 / |legal|. With it a search is the
 * batched counterpart of game.py:294-379's mcts_action (PUCT over uniform priors in place of UCB1). A function of the
 * position and the seed alone, so exact under the evaluation cache. */
int uttt_eval_playout_dev(uttt_engine_t *eng, int32_t playouts, uint64_t seed, float *policy, float *value);
/* uttt_playout_host on the device, one wave per state (game.py:277-287 for n states at once; terminal states
 * included): copies the states in, runs on the engine's stream, copies the counts out and synchronises.
 * states, wins, losses: host memory. Independent of any search in progress. */
int uttt_playouts(uttt_engine_t *eng, const uttt_state_t *states, int32_t n, int32_t playouts, uint64_t seed,
                  int32_t *wins, int32_t *losses);
/* uttt_solve_host on the device (game.py:240-274 for n positions at once), one wave per position and one
 * lane per legal move: copies the states in, runs on the engine's stream, copies the results out and
 * synchronises. All pointers are host memory; any output may be NULL. Independent of any search in progress. */
int uttt_solve(uttt_engine_t *eng, const uttt_state_t *states, int64_t n, int32_t max_nodes, int8_t *value,
               int8_t *action, int8_t *status, int64_t *nodes, int8_t *action_values);
/* uttt_solve_overlay_host on the round's pending leaves (the count read on the device, as
 * uttt_eval_playout_dev; after uttt_search_select or uttt_search_select_async), run after any evaluator has
 * filled the rows and before the apply: row r of policy (at policy + r * policy_ld, policy_ld >= 81) and
 * value[r * value_ld] get the exact value, and with UTTT_PRIORS_OPTIMAL the marks of the optimal moves, of
 * every leaf with at most max_empties empties that max_nodes per move proves; the other rows keep what the
 * evaluator wrote. status: int8 per row (device memory), may be NULL. One wave per leaf on the engine's
 * stream. The overlay is a function of the position and the three parameters alone, so a search stays exact
 * under the evaluation cache as long as the parameters do not change while a table is warm (clear it when
 * they do). One row per leaf: per-copy applies are out of scope. */
int uttt_eval_solve_dev(uttt_engine_t *eng, int32_t max_empties, int32_t max_nodes, int32_t priors, float *policy,
                        int64_t policy_ld, float *value, int64_t value_ld, int8_t *status);
/* The round's pending leaves seen through a symmetry (the count read on the device, as uttt_eval_playout_dev;
 * after uttt_search_select or uttt_search_select_async): states_out[r] = T_g(leaf r), sym_out[r] = g, and,
 * unless nn_input_out is NULL, row r of nn_input_out = the NCHW (3, 9, 9) network input of T_g(leaf r).
 * mode UTTT_SYM_FIXED: g = g_or_seed (0..7) for every leaf; UTTT_SYM_HASHED: g = uttt_states_symmetry_host's
 * choice for the leaf with seed g_or_seed. states_out: max_trees states, sym_out: max_trees int8,
 * nn_input_out: max_trees * 243 f32, device memory; rows past the count are untouched. One wave per leaf on
 * the engine's stream. */
#define UTTT_SYM_FIXED 0
#define UTTT_SYM_HASHED 1
int uttt_sym_pending_dev(uttt_engine_t *eng, int32_t mode, uint64_t g_or_seed, uttt_state_t *states_out,
                         int8_t *sym_out, float *nn_input_out);
/* An evaluator's rows for transformed leaves mapped back (the count read on the device, as above): for row r
 * below the count and g = sym[r],
 *   out_policy[r * out_policy_ld + a] = (policy[r * policy_ld + pi_g(a)] [+ out_policy[...] if accumulate]) [* scale]
 *   out_value[r * out_value_ld]       = (value[r * value_ld]             [+ out_value[...]  if accumulate]) [* scale]
 * in f32, the multiplication only when scale != 1. Without accumulate the row is a plain permuted copy. No
 * output buffer may overlap an input buffer (checked over one row per tree of the search: UTTT_ERR_ARG); the
 * leading dimensions of the policies are >= 81, the value
 * strides >= 1 (as uttt_eval_solve_dev). Rows past the count are untouched. One wave per row on the engine's
 * stream. */
int uttt_sym_rows_dev(uttt_engine_t *eng, const int8_t *sym, const float *policy, int64_t policy_ld,
                      const float *value, int64_t value_ld, float *out_policy, int64_t out_policy_ld,
                      float *out_value, int64_t out_value_ld, int32_t accumulate, float scale);
/* One whole round with the hash evaluator, enqueued by one call (round 5; the rounds of
 * SelfPlay.steps with HashEvaluator lanes, i.e. the kernel microbenchmark of SURVEY §8(d)):
 * uttt_search_select_async_tag(ring_slot, tag) -> uttt_eval_hash_dev(policy, value) ->
 * uttt_search_apply(on_device), with the apply staged: the next call runs it, its own select and its
 * own evaluation as one launch (k_round1: per tree, the previous evaluation applied, then the next
 * descent, then the queued leaf evaluated into the tree's row), and any other call that reads the
 * trees (the move's end, the root results, a synchronous select) applies it first.
 * UTTT_FUSED_ROUNDS=0 launches the three steps as written above. The round stores its
 * counts and then `tag` (word 3 of the slot; the counts' stores drained before it), so the host
 * learns that the counts landed by polling the tag: no event and no host sync per round. policy:
 * (max_trees, 81) f32, value: (max_trees,) f32, device memory, left untouched until the staged apply
 * has run. Replaces, for the test evaluator, one pass of the flush loop of uttt_mcts.cpp:109-167
 * over every tree. */
int uttt_round_hash_async(uttt_engine_t *eng, int32_t ring_slot, int32_t tag, float *policy, float *value);
/* n_rounds consecutive rounds in one call (round 6, tree-only self-play: the host's per-round reaction was
 * the bound): ring slots ring_slot .. ring_slot + n_rounds - 1 (mod 8) and tags tag .. tag + n_rounds - 1;
 * a round past the move's last finds every tree done and changes nothing. */
int uttt_rounds_hash_async(uttt_engine_t *eng, int32_t ring_slot, int32_t tag, float *policy, float *value,
                           int32_t n_rounds);
/* A move's whole round loop in one call (round 6; replaces, for the test evaluator, the flush loop of
 * uttt_mcts.cpp:109-167 run to the move's end over every tree, as self_play_cpp.play's per-move
 * pv_mcts_scores call does): `depth` hash rounds kept in flight (uttt_round_hash_async, ring slots from
 * ring_slot on, tags tag, tag + 1, ... masked to 31 bits), the host spinning on each round's tag in turn and
 * enqueueing the next until a round reports no tree with simulations left. Returns when that round's
 * counts landed; the rounds still in flight behind it are empty. *n_rounds: rounds enqueued (ring slots and
 * tags consumed), *n_leaves: leaves evaluated, *n_with_leaves: rounds that had leaves. */
int uttt_rounds_hash_move(uttt_engine_t *eng, int32_t ring_slot, int32_t tag, float *policy, float *value,
                          int32_t depth, int32_t *n_rounds, int64_t *n_leaves, int32_t *n_with_leaves);

/* Root results after the search: visit counts of the root's children (legal
 * order, row stride 81) and |legal| per tree. */
int uttt_search_root_visits(uttt_engine_t *eng, int32_t *visits, int32_t *n_legal);
/* Scores as pv_mcts_scores returns them (uttt_mcts.cpp:177-195): one-hot first
 * max for temperature 0, else boltzman; row stride 81. */
int uttt_search_scores(uttt_engine_t *eng, float temperature, float *scores, int32_t *n_legal);

/* The priors P of the root's children (legal order, row stride 81, zeros past |legal|) and |legal| per tree,
 * any time after the search began: 1.0f / |legal| unless root noise is on. Either output may be NULL. */
int uttt_search_root_priors(uttt_engine_t *eng, float *priors, int32_t *n_legal);
/* Root exploration noise: with epsilon > 0 every root built from then on by uttt_search_begin,
 * uttt_search_begin_mode(UTTT_SEMANTICS_CPP) or a self-play move begin (blocking or _async) gets the priors
 * uttt_root_noise_host describes, written by one extra launch (k_root_noise) behind the one that builds the
 * roots. epsilon 0 (the default) is off: no launch, today's priors. While it is on,
 * uttt_search_begin_mode(UTTT_SEMANTICS_PY) and uttt_search1_begin return UTTT_ERR_ARG (a py root's priors come
 * from its first flush; the resident one-tree search builds its root inside its own kernel). UTTT_ERR_ARG for
 * epsilon outside [0, 1] or alpha outside [1/32, 32] (alpha is checked even when epsilon is 0). */
int uttt_engine_set_root_noise(uttt_engine_t *eng, float epsilon, float alpha, uint64_t seed);

/* Tree reuse (off by default): with it on, a self-play move begin (blocking, _async, and the move
 * loops built on them) builds each slot's root by k_reroot in place of k_begin. For a live slot whose game
 * continues, the root's child c with the action the slot played (ply_action[slot][ply - 1]) becomes the new root
 * and the subtree under it is kept: c's link.k duplicate child sets are merged move by move into one block (N and
 * link.k summed, W summed in f32 in copy order, P of the first copy: the evaluator's priors, where a fresh root has
 * 1 / |legal|; the copies' child blocks concatenated in copy order), everything below is copied with re-based
 * first-child indices, and the pool is laid out breadth first (root, its block, then the child blocks of the nodes
 * in the order the nodes stand). The new root's record: N = N_c - k_c (the sum of its children's visits), W as
 * c's (nothing reads a root's W), P 0, no action, link (1, 1). The search starts with sims_done = N_c - k_c, so a
 * move tops the root up to evaluate_count visits instead of adding evaluate_count: root visits still sum to
 * evaluate_count and the pool's bound 82 + 81 * max_sims holds. A slot that is not live, holds a new game, or
 * whose c has no children (never expanded, or terminal) gets the fresh root k_begin writes. Root noise, when on,
 * is mixed into the carried priors. The trees are copied into a second node pool as large as the first,
 * allocated when reuse is first switched on and counted by uttt_engine_device_bytes; the two change places every
 * move. While it is on, uttt_search_begin_mode(UTTT_SEMANTICS_PY) and uttt_search1_begin return UTTT_ERR_ARG (a py
 * tree's expansions replace; the resident one-tree search keeps its tree in its own wave). It may be called at
 * any time and holds from the next move begin on. */
int uttt_engine_set_tree_reuse(uttt_engine_t *eng, int32_t on);
/* Re-root every tree of a finished uttt_search_begin search (C++ semantics, every leaf applied) at actions[t],
 * as above, and begin the next search on the carried trees: each runs until its root has evaluate_count visits
 * (at least the finished search's evaluate_count; the batch size stays). Then select / apply rounds as after
 * uttt_search_begin. UTTT_ERR_ARG for an action that is -1 or not a legal move of its tree's root (nothing is
 * changed then), and after a search with Python semantics; UTTT_ERR_ORDER while tree reuse is off. */
int uttt_search_reroot(uttt_engine_t *eng, const int32_t *actions, int32_t evaluate_count);
/* One tree's node records, four uint32 each (W f32 bits, P f32 bits, meta = N : 16 | action : 7 | L : 7 | 2 flags,
 * link = first child : 20 | k : 12; the root is record 0): *node_count records are copied to `records` (room for
 * `cap` records; NULL: only the count). For tests and analysis; synchronises the stream. */
int uttt_search_tree(uttt_engine_t *eng, int32_t tree, uint32_t *records, int32_t cap, int32_t *node_count);
/* What uttt_search_reroot / a reusing move begin makes of one tree, in plain C++ (csrc/uttt_reroot.h): records
 * (node_count of them, as uttt_search_tree gives them) of a tree whose root's position is *state, re-rooted at
 * `action`, to out (room for max(node_count, 82) records) and *out_count, bit for bit what the device writes.
 * UTTT_ERR_ARG for an action that is not a move of the root. Pure CPU. */
int uttt_reroot_host(const uint32_t *records, int32_t node_count, const uttt_state_t *state, int32_t action,
                     uint32_t *out, int32_t *out_count);

/* ------------------------------------------------------------------ match --- */
/* A match between two players with every game resident on the device (csrc/uttt_match.h): the
 * loop of evaluate_network.py:78-92 over play() (:33-54), each player an engine of its own. Game g starts at
 * openings[g / 2] when the match is paired and at openings[g] when not, and player g % 2 takes the side to move
 * at the start position (:82-85: the players swap from game to game), so games 2 i and 2 i + 1 are one opening
 * with the colours swapped. Per game the match holds the position, the ply counted from the start position, the
 * actions played and a result: -1 while the game is live, else player 0's half-points 0 / 1 / 2 (:26-30 times
 * two, from player 0's side as :83 / :85 count them).
 *
 * One iteration of the caller's loop: uttt_match_counts; for each player whose list is not empty
 * uttt_match_search_begin, the ordinary select / evaluator / apply rounds on that player's engine, and
 * uttt_match_move; then uttt_match_lists. The match ends when both lists are empty. Both engines run on the
 * stream given to uttt_match_begin (uttt_engine_set_stream).
 *
 * Out of scope, and refused by uttt_match_search_begin with UTTT_ERR_ARG while they are on: root noise (a plain
 * search keys it by tree index, which here changes from ply to ply) and tree reuse. */
typedef struct uttt_match uttt_match_t;
/* Room for max_games games (1 .. 2^20 - 1) on `device` (-1 = the calling thread's current device). */
int uttt_match_create(int32_t device, int32_t max_games, uttt_match_t **out);
int uttt_match_destroy(uttt_match_t *m);
/* The argument check of uttt_match_begin, pure CPU: UTTT_ERR_ARG with a message for a NULL or terminal opening
 * (:43 would end such a game before its first move), games outside 1..max_games, `paired` with an odd `games`,
 * and n_openings below what the games need (games / 2 when paired, else games). */
int uttt_match_check_host(const uttt_state_t *openings, int32_t n_openings, int32_t games, int32_t max_games,
                          int32_t paired);
/* Start a match (:33-38's initial state, for every game at once): openings are host states; moves at a ply below
 * sample_plies are drawn in proportion to the visit counts with `seed`, later ones are the most visited move.
 * `stream`: a hipStream_t (NULL = the null stream). Builds the first lists; synchronises the stream. */
int uttt_match_begin(uttt_match_t *m, const uttt_state_t *openings, int32_t n_openings, int32_t games, int32_t paired,
                     int32_t sample_plies, uint64_t seed, void *stream);
/* Synchronises the stream and returns out[0..4] = {games in which player 0 is to move, games in which player 1
 * is, games finished, player 0's half-points over the finished games, finished games that were drawn}
 * (:79-92's total_point, kept in integers). */
int uttt_match_counts(uttt_match_t *m, int64_t out[5]);
/* Begin a plain search of `eng` on the positions of `player`'s list (:47-48: the player to move searches), device
 * to device: uttt_search_begin_mode's checks and root kernel, with the tree count the list length that
 * uttt_match_counts last returned; tree t is the t-th game of the list. UTTT_ERR_ORDER if the lists are stale (no
 * uttt_match_counts since uttt_match_lists, or `player` has moved since); UTTT_ERR_ARG for an empty list, an
 * engine on another stream or device, and root noise or tree reuse on. Then select / evaluator / apply rounds. */
int uttt_match_search_begin(uttt_match_t *m, uttt_engine_t *eng, int32_t player, int32_t evaluate_count,
                            int32_t batch_size, int32_t semantics);
/* Play the searched move in every game of `player`'s list (:48-51): the search begun by uttt_match_search_begin
 * on `eng` must have every leaf applied; a failed tree is reported here, as by uttt_search_root_visits. Launches
 * the root-visit kernel and k_match_move on the engine's stream and returns at once. UTTT_ERR_ORDER without that
 * search, and for a second move of `player` before uttt_match_lists. */
int uttt_match_move(uttt_match_t *m, uttt_engine_t *eng, int32_t player);
/* Rebuild both players' lists and root arrays and the counters (:41-44: finished games leave the loop). Once per
 * iteration, after both players have moved; returns at once. */
int uttt_match_lists(uttt_match_t *m);
/* Host copies of the games' state: results[g] (int8: -1 live, else player 0's half-points), plies[g], actions
 * [g][81] (int8, -1 past the ply) and states[g]. Any pointer may be NULL. Synchronises the stream. */
int uttt_match_games(uttt_match_t *m, int8_t *results, int32_t *plies, int8_t *actions, uttt_state_t *states);
/* The move rule in plain C++ (csrc/uttt_match.h), bit for bit what k_match_move writes (:48-51 for one game):
 * visits are the root's n_visits counts in legal order (n_visits must be the state's legal count, counts
 * non-negative); *next, *action and *result (-1, or player 0's half-points) are written. Pure CPU. UTTT_ERR_ARG
 * for a terminal state, a row of another length, a negative count, or a ply outside 0..80. */
int uttt_match_move_host(const uttt_state_t *state, const int32_t *visits, int32_t n_visits, int32_t ply,
                         int64_t game, uint64_t seed, int32_t sample_plies, uttt_state_t *next, int32_t *action,
                         int32_t *result);
/* The 64-bit draw of (seed, game, ply) that a sampled move of :48 uses in place of np.random.choice's. Pure CPU. */
uint64_t uttt_match_draw_host(uint64_t seed, int64_t game, int32_t ply);

/* -------------------------------------------------------------- self-play --- */
/* Self-play of games [game_begin, game_end) (self_play_cpp.py:34-130), each
 * game g with its own numpy-legacy MT19937 seeded seed_base + g (=
 * np.random.seed(seed_base + g) before self_play_cpp.play). Slots are refilled
 * with the next game id as games end. arena_plies bounds the finished-game
 * record arena (plies). */
int uttt_selfplay_begin(uttt_engine_t *eng, int64_t game_begin, int64_t game_end, uint32_t seed_base,
                        float temperature, int32_t evaluate_count, int32_t batch_size, int64_t arena_plies);
/* Start one move for every live game: its search tree is rebuilt from the
 * current position (uttt_mcts.cpp:92 has no tree reuse; uttt_engine_set_tree_reuse
 * carries the played move's subtree over instead). *n_live = live slots
 * (0 = every game finished). Then run select/eval/apply rounds. */
int uttt_selfplay_move_begin(uttt_engine_t *eng, int32_t *n_live);
/* Finish the move (self_play_cpp.py:63-92): scores -> f64 policy target
 * (np.sum renormalisation) -> np.random.choice -> record -> next state;
 * ended games get their values (self_play_cpp.py:95-99) and are written to
 * the arena; free slots take the next game. *n_finished = games in the arena. */
int uttt_selfplay_move_end(uttt_engine_t *eng, int64_t *n_finished);
/* A temperature schedule for self-play: a move made at ply < plies uses uttt_selfplay_begin's temperature, a
 * later one late_temperature (0 = the most visited move), for the sampled move and the recorded policy target
 * alike. A setting of the engine: call it before or after uttt_selfplay_begin, between moves (UTTT_ERR_ORDER
 * between a self-play move's begin and its end); it holds for every move end enqueued afterwards and across
 * later uttt_selfplay_begin calls. The default, plies = INT32_MAX, is one temperature for the whole game.
 * UTTT_ERR_ARG for plies < 0 or a late_temperature that is negative or not finite. */
int uttt_selfplay_set_temperature_schedule(uttt_engine_t *eng, int32_t plies, float late_temperature);
/* numpy-legacy MT19937 state of a slot's current game (624 words + position),
 * so a caller can run a game on numpy's global RandomState and continue it
 * afterwards (self_play_cpp.play draws from np.random, self_play_cpp.py:86). */
int uttt_selfplay_get_rng(uttt_engine_t *eng, int32_t slot, uint32_t key[624], int32_t *pos);
int uttt_selfplay_set_rng(uttt_engine_t *eng, int32_t slot, const uint32_t key[624], int32_t pos);
/* The move boundary without host synchronisation, for a driver that pipelines moves
 * (DESIGN.md §7): uttt_selfplay_move_end_async enqueues the move's end (scores, sampled move,
 * records, new games for free slots) and a copy of the counters to pinned host memory;
 * uttt_selfplay_move_begin_async enqueues the next move's roots (the live flags stay on the
 * device). Once the stream has passed that copy (e.g. an event recorded after it completed),
 * uttt_selfplay_move_result reports failed trees and a full arena, as move_end does, and
 * returns the games finished so far and the live slots of the next move. Not with periodic
 * cache clears (uttt_engine_set_cache clear_every > 0). */
int uttt_selfplay_move_begin_async(uttt_engine_t *eng);
int uttt_selfplay_move_end_async(uttt_engine_t *eng);
int uttt_selfplay_move_result(uttt_engine_t *eng, int64_t *n_finished, int32_t *n_live_next);

/* Finished games: n_games entries of (game id, first ply in arena, plies),
 * sorted by game id; then the arena rows [0, n_plies): state, policy target
 * (81 f64), action, value. Any output pointer may be NULL. */
int uttt_selfplay_games(uttt_engine_t *eng, int64_t *game_ids, int64_t *offsets, int32_t *lengths,
                        int64_t max_games, int64_t *n_games);
int uttt_selfplay_plies(uttt_engine_t *eng, uttt_state_t *states, double *policies, int8_t *actions,
                        int8_t *values, float *inputs_hwc, int64_t max_plies, int64_t *n_plies);

/* ----------------------------------------------------- evaluation cache --- */
/* Use `owner`'s evaluation table instead of a private one (several engines on
 * one GPU, e.g. SelfPlay lanes, then see each other's evaluations). Lookups and
 * inserts are coherent across concurrently running kernels; only the owner
 * clears the table (its clear_every_moves). The owner must outlive `eng`. */
int uttt_engine_share_cache(uttt_engine_t *eng, uttt_engine_t *owner);
/* Position -> raw evaluator output table in HBM (2^log2_capacity entries of
 * 360 B; 0 = off, the default). A flushed leaf whose position is cached is
 * expanded from the table inside the select kernel instead of waiting for the
 * evaluator. Exact for a deterministic evaluator (the evaluator sees only the
 * position, uttt_game.cpp:244-280). Self-play clears it at begin and every
 * clear_every_moves moves (0 = never); per-copy apply bypasses it. */
int uttt_engine_set_cache(uttt_engine_t *eng, int32_t log2_capacity, int32_t clear_every_moves);
int uttt_engine_cache_clear(uttt_engine_t *eng);
/* hits: leaves resolved from the table; misses: leaves sent to the evaluator. */
int uttt_engine_cache_stats(uttt_engine_t *eng, int64_t *hits, int64_t *misses, int64_t *inserts);
/* The same plus replacements: inserts that found every probe slot holding another position and
 * rewrote one of them (a full probe window; readers of the old entry retry). */
int uttt_engine_cache_stats2(uttt_engine_t *eng, int64_t *hits, int64_t *misses, int64_t *inserts,
                             int64_t *replacements);

/* ------------------------------------------------------------ telemetry --- */
/* Per-kernel timing with HIP events on the engine's stream (off by default). */
int uttt_engine_set_timing(uttt_engine_t *eng, int32_t enabled);
/* kernel: 0 select, 1 apply, 2 encode, 3 scan, 4 move_end, 5 hash_eval, 15 playout, 16 solve,
 * 17 solve_leaves, 18 sym_leaves, 19 sym_rows, 20 root_noise, 21 reroot.
 * Outputs total ms, launches and algorithmic bytes. Counters without launches
 * (value in *algo_bytes): 6 tree levels walked by select (sum over descents of depth + 1),
 * 7 trees that descended, 9 sum over select launches of the slowest tree's levels. */
int uttt_engine_kernel_stats(uttt_engine_t *eng, int32_t kernel, double *total_ms, int64_t *launches,
                             int64_t *algo_bytes);
int uttt_engine_reset_stats(uttt_engine_t *eng);

#ifdef __cplusplus
}
#endif

#endif /* UTTT_ENGINE_H */
