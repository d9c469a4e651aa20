"""Rank process of tests/test_eval_cpu.py (gloo, CPU): all-reduces an evaluation run state and prints it."""
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dcanet_amd  # noqa: E402,F401
from dcanet_amd.evaluation import STATE_HEAD, all_reduce_state  # noqa: E402
from dcanet_amd.parallel import init_from_env  # noqa: E402

rank, _, world = init_from_env("gloo")
C = 24
state = torch.from_numpy(np.random.RandomState(40 + rank).rand(STATE_HEAD + 3 * C * C) * 1e6)
state[STATE_HEAD:] = state[STATE_HEAD:].floor()              # counts
out = all_reduce_state(state)
assert out is state
print("RESULT " + json.dumps(state.tolist()), flush=True)
dist.barrier()
dist.destroy_process_group()
