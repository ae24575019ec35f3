"""train() on the cube, synchronous loop, three outer iterations, run three times in one process after different contents were
left in the allocator's cache -- eager launches against graph-captured sub-steps, per stepper family.  Shows that graph-captured
training on the slow stepper families (generic path, tiled family) departs from eager launches from the third outer iteration on,
while the MFMA containers agree.  python tools/train_graph_repro.py [mfma|generic|tiled] [graphs|eager]"""
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import configs.Ex4_1_funcs as P                              # noqa: E402
from src.training import NODE_WAN_solver                     # noqa: E402
from xnode_wan_pde_solver_amd.options import EngineOptions   # noqa: E402

WIDTHS = {'mfma': (20, 10, 8), 'generic': (48, 16, 11), 'tiled': (128, 32, 8)}


def run(H, K, m, graphs, seed=4):
    params = {'alpha': 1e3, 'u_layers': m, 'u_hidden_dim': H, 'u_hidden_hidden_dim': K, 'v_layers': 4, 'v_hidden_dim': 50,
              'n1': 2, 'n2': 1, 'u_rate': 0.015, 'v_rate': 0.04, 'min_steps': 5, 'adjoint': False, 'solver': 'midpoint',
              'dim': 5, 'N_t': 7, 'N_r': 200, 'N_b': 100, 'T0': 0, 'T': 1, 'shape_param': [-1, 1], 'iterations': 3,
              'domain': 'Hypercube'}
    torch.manual_seed(seed)
    np.random.seed(seed)
    S = NODE_WAN_solver(params, P.func_a, P.func_b, P.func_c, P.func_h, P.func_f, P.func_g, torch.device('cuda'), './',
                        func_u_sol=P.func_u_sol, p=2, options=EngineOptions(use_graphs=graphs))
    S.pipeline = S.overlap_sampling = False
    cwd = os.getcwd()
    os.chdir(tempfile.mkdtemp())
    try:
        return [float(v) for v in S.train(report=False)]
    finally:
        os.chdir(cwd)


if __name__ == '__main__':
    fam, mode = sys.argv[1], sys.argv[2]
    for junk in (float('nan'), 0.0, 1.0):
        x = torch.full((1 << 27,), junk, dtype=torch.float64, device='cuda')
        del x
        print(fam, mode, run(*WIDTHS[fam], mode == 'graphs'), flush=True)
