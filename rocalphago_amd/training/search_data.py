"""Search-generated policy targets: self-play with ParallelMCTS, every position recorded with
the root's visit counts.

The output is the SGF converter's dataset (``states`` uint8 [N, F, S, S], ``actions`` uint8
[N, 2] = the move played, ``features``) plus ``visits``: uint16 [N, S*S + 1], the root children's
visit counts of the search that chose the move (pass last, saturating at 65535), and
``outcomes``: int8 [N], the game's result for the player to move at that position (+1 won, -1
lost, 0 drawn; the engine's ``get_winner()`` at the end of the game or at the move limit): the
value targets of a policy-value network (``supervised.py`` with a CNNPolicyValue). Training on the
normalised rows (``supervised.py --targets visits``) is the AlphaGo Zero / expert-iteration policy
target; ``--targets actions`` on the same file trains on the moves alone. Positions where the move
played is a pass are skipped, as the converter skips them.

Every position is searched from a fresh tree, so a row sums to at most ``--playouts``. The loop
is sequential: one game, one position at a time (the search itself is batched on the GPU).

    python -m rocalphago_amd.training.search_data policy.json out.h5 --games 100 --playouts 800
"""
import numpy as np

from ..engine import gamestate as go
from ..features.preprocessing import DEFAULT_FEATURES, Preprocess
from ..io import h5lite


def visit_row(moves, visits, size):
    """Root statistics -> uint16 [S*S + 1] counts (a move < 0 is the pass, stored last)."""
    P = size * size
    row = np.zeros(P + 1, np.int64)
    for m, v in zip(moves, visits):
        row[P if m < 0 else int(m)] += int(v)
    return np.minimum(row, 65535).astype(np.uint16)


def choose_move(row, rng, sample):
    """Index into a visit row: drawn in proportion to the counts (``sample``), else the most
    visited (lowest index on ties). None when the row is empty."""
    total = int(row.astype(np.int64).sum())
    if total == 0:
        return None
    if sample:
        return int(rng.choice(len(row), p=row.astype(np.float64) / total))
    return int(np.argmax(row))


def play_game(mcts, size, rng, temperature_moves=0, move_limit=None):
    """One self-play game; returns the recorded (states, actions [n, 2], visits [n, S*S + 1],
    outcomes int8 [n]: the game's result for the player to move at each recorded position)."""
    P = size * size
    move_limit = move_limit or 2 * P
    state = go.GameState(size=size)
    states, actions, rows = [], [], []
    while not state.is_end_of_game and len(state.history) < move_limit:
        mcts.reset()
        mcts.search(state)
        mvs, vis, _, _ = mcts.root_statistics()
        row = visit_row(mvs, vis, size)
        a = choose_move(row, rng, len(state.history) < temperature_moves)
        if a is None or a == P:
            state.do_move(go.PASS_MOVE)
            continue
        move = divmod(a, size)
        states.append(state.copy())
        actions.append(move)
        rows.append(row)
        state.do_move(move)
    winner = state.get_winner()
    outcomes = np.asarray([0 if winner == 0 else (1 if st.current_player == winner else -1)
                           for st in states], np.int8)
    return states, np.asarray(actions, np.uint8).reshape(-1, 2), \
        np.asarray(rows, np.uint16).reshape(-1, P + 1), outcomes


def generate_search_data(mcts, n_games, out_file, size=19, features=DEFAULT_FEATURES,
                         temperature_moves=0, seed=0, move_limit=None, verbose=False):
    """Play ``n_games`` with ``mcts`` (a search.apv.ParallelMCTS) and write ``out_file``; returns
    the number of positions written."""
    pp = Preprocess(features)
    rng = np.random.RandomState(seed)
    shp = (pp.output_dim, size, size)
    P1 = size * size + 1
    n = 0
    with h5lite.File(out_file, "w") as f:
        ds = f.create_dataset("states", shape=(0,) + shp, dtype=np.uint8, maxshape=(None,) + shp,
                              chunks=(64,) + shp, compression="lzf")
        da = f.create_dataset("actions", shape=(0, 2), dtype=np.uint8, maxshape=(None, 2),
                              chunks=(1024, 2), compression="lzf")
        dv = f.create_dataset("visits", shape=(0, P1), dtype=np.uint16, maxshape=(None, P1),
                              chunks=(256, P1), compression="lzf")
        do = f.create_dataset("outcomes", shape=(0,), dtype=np.int8, maxshape=(None,),
                              chunks=(4096,), compression="lzf")
        f["features"] = np.bytes_(",".join(features))
        for g in range(n_games):
            states, actions, rows, outcomes = play_game(mcts, size, rng, temperature_moves,
                                                        move_limit)
            if states:
                ds.append(pp.states_to_tensor_u8(states))
                da.append(actions)
                dv.append(rows)
                do.append(outcomes)
                n += len(states)
            if verbose:
                print("game %d: %d positions (%d in all)" % (g, len(states), n))
    return n


def run(cmd_line_args=None):
    import argparse
    parser = argparse.ArgumentParser(
        description="Self-play with MCTS; write positions with the root visit counts.")
    parser.add_argument("policy", help="Path to a policy model JSON (with its weights_file)")
    parser.add_argument("out_file", help="The .h5 dataset to write")
    parser.add_argument("--games", type=int, default=10, help="Games to play. Default: 10")
    parser.add_argument("--playouts", type=int, default=800,
                        help="Simulations per position. Default: 800")
    parser.add_argument("--size", type=int, default=19, help="Board size. Default: 19")
    parser.add_argument("--value", default=None,
                        help="Path to a value model JSON (default: rollouts only; omit it with "
                             "a policy-value network as policy, whose own value head is searched "
                             "with)")
    parser.add_argument("--seed", type=int, default=0, help="Seed of the search and the sampling")
    parser.add_argument("--temperature-moves", type=int, default=0,
                        help="The first so many plies are drawn in proportion to the visit "
                             "counts, the rest take the most visited move. Default: 0")
    parser.add_argument("--verbose", "-v", default=False, action="store_true")
    args = parser.parse_args(cmd_line_args)

    from ..models.policy import CNNPolicy
    from ..models.policy_value import CNNPolicyValue
    from ..models.value import CNNValue
    from ..search.apv import ParallelMCTS
    policy = CNNPolicy.load_model(args.policy)
    if policy.model.input_shape[-1] != args.size:
        raise ValueError("the policy plays %dx%d boards, --size is %d" %
                         (policy.model.input_shape[-1], policy.model.input_shape[-1], args.size))
    if isinstance(policy, CNNPolicyValue) and args.value:
        raise ValueError("a policy-value network searches with its own value head: omit --value")
    value = CNNValue.load_model(args.value) if args.value else None
    mcts = ParallelMCTS(policy, value, n_playout=args.playouts, seed=args.seed)
    n = generate_search_data(mcts, args.games, args.out_file, size=args.size,
                             features=policy.preprocessor.feature_list,
                             temperature_moves=args.temperature_moves, seed=args.seed,
                             verbose=args.verbose)
    if args.verbose:
        print("%d positions written to %s" % (n, args.out_file))
    return n


if __name__ == "__main__":
    run()
