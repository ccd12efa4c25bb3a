"""AlphaGo.training.search_data (not in the reference) — MCTS self-play positions with root
visit counts. See rocalphago_amd/training/search_data.py."""
from rocalphago_amd.training.search_data import generate_search_data, run  # noqa: F401

if __name__ == '__main__':
    run()
