"""The fused XNODE-WAN training step: generator and discriminator sub-steps as explicit sequences of HIP kernels.

Replaces the bodies of the two sub-step loops of NODE_WAN_solver.train (src/training.py:125-138,151-162 of the
reference): forward of both nets, func_eval, loss.u / loss.v with their three autograd backward passes, and
optimizer.step().  No autograd tape is built; every gradient is an explicit kernel (xw_ode_bwd, xw_disc_bwd).

Semantics are the reference's ON A GPU, stated once here and implemented literally below:
  Q1  the helper backwards of loss.I also deposit d(sum u)/dtheta resp. d(sum phi)/dphi in the parameter gradients
      -> `pollution = 1` in the cotangent kernels (set Engine.pollution = 0.0 for the textbook gradient);
  Q2  nabla u, nabla phi enter I as constants; the u-factor of the d(phi)/dt term carries no gradient;
  Q3  nabla_x u is the time-summed input gradient G_n = d(sum_l u[n,l])/dx_n (incl. the path through h(x)), seen at
      time index 0 only -> the a_ij contraction is per path (s3x);
  Q4  v is evaluated on its own interior sample XV;
  Q5  no stale .grad carry-over between sub-steps (that is a CPU-only artefact of the reference).

The per-sample half -- loading a sample into a Group, the data layout of a group in HBM -- is groups.py (GroupLoading, the
base class of Engine); this file is the sub-step schedule: streams, graphs, the runner, both sub-steps and predict*.
"""
import contextlib

import torch

from . import kernels as KN
from ._lib import XnwanError
from .options import EngineOptions
from .groups import F32, F64, Group, GroupLoading, Structure, at_T0, start_values      # noqa: F401  (Group, Structure: part of this module's surface)
from .sampling import HIP_HOST_LOCK


def ctypes_addr(fn):
    """address of a ctypes callback object (kept alive by the caller)"""
    import ctypes
    return ctypes.cast(fn, ctypes.c_void_p).value

# Every captured sub-step graph of the process, kept alive until it exits.  On this stack (ROCm 7.2 runtime inside the
# PyTorch 2.10 wheel) destroying the executable of a multi-branch graph -- which is what Python's garbage collector does to
# the graphs of a solver that went out of scope -- leaves the runtime's per-graph stream bookkeeping in a state in which a
# LATER launch of another, live graph dereferences a dead stream: SIGSEGV in hip::Graph::UpdateStreams under
# hipGraphLaunch (rocgdb backtrace, round 3; it took a particular sequence of 27 tests to line the collector up with a
# replay).  Collecting before a new engine captures does not help; not destroying does.  A graph is a few dozen kernel
# nodes and holds no sample buffers (those belong to the group), so the cost of keeping it is small.
_KEPT_GRAPHS = []

_NOSTREAM = contextlib.nullcontext()      # Engine._side without side streams

# One private memory pool for the captured graphs that ALLOCATE while they are recorded (the training loop's refill of its
# group, its diagnostic: path tensors and the temporaries of the user's callables, ~100 MB at the headline size).  Their
# results are copied into buffers of the group inside the graph, nothing in the pool is read after a replay has ended, and
# replays are issued on one stream: the graphs of every group and solver of the process can reuse the same memory -- kept
# graphs (above) then cost their nodes, not a pool each.
_SCRATCH_POOL = []


# The side streams and the capture stream are per DEVICE, shared by every engine of the process (engines are driven from one
# host thread and never run concurrently): the allocator only reuses a block on the stream it was allocated on, so with
# streams per engine the scratch pool above grew by what one refill allocates (54 MB at the headline size) per solver.
_DEVICE_STREAMS = {}


def _device_streams(device):
    key = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    if key not in _DEVICE_STREAMS:
        _DEVICE_STREAMS[key] = ([torch.cuda.Stream(device=device) for _ in range(4)], torch.cuda.Stream(device=device))
    return _DEVICE_STREAMS[key]


def _scratch_pool(which=0):
    """which: graphs that may be replayed CONCURRENTLY (the diagnostic of one outer iteration beside the refill for the next one,
    solver._iterate_pipelined) must not share scratch memory -- pool 0: refills, pool 1: diagnostics"""
    while len(_SCRATCH_POOL) <= which:
        _SCRATCH_POOL.append(torch.cuda.graph_pool_handle())
    return _SCRATCH_POOL[which]


class Engine(GroupLoading):
    def __init__(self, config, setup, u_mod, v_mod, funcs, device, world=None, structure=None, options=None):
        self.config, self.setup, self.u, self.v, self.funcs, self.dev, self.world = config, setup, u_mod, v_mod, funcs, device, world
        # every switch comes from ONE object (options.EngineOptions; the XW_* environment is read once, in from_env()); the
        # attributes below are the working copies -- tests and tools set them directly
        opt = self.options = options if options is not None else EngineOptions.from_env()
        KN.apply_switches(opt)          # the library's process-wide switches: this engine's, until another one is built (options.py)
        self.d = setup['dim']
        self.method = KN.method_id(config['solver'])
        # solver 'dopri5' (DESIGN 8): every forward reads its step controllers back to the host between chunks of attempts, so
        # no segment that holds one can be captured -- decided here, up front: eager launches on one stream, no fused runner
        # (xw_substep_* is fixed-grid), no activation store (the sweeps recompute from the step record)
        self.dopri5 = self.method == KN.DOPRI5
        self.dopri5_stepper = KN.dopri5_stepper(opt.dopri5_stepper)     # 'vector' | 'tiled': which kernels run its field
        self._dopri_recs = {}
        if self.dopri5 and world is not None:
            raise XnwanError("solver 'dopri5' runs on one GPU: its step sizes are per group and chosen on the device, and a "
                             "group sharded over %d ranks would need an exchange per attempted step (not built)" % world.size)
        # config['adjoint'] (src/model.py:103): the sweeps integrate torchdiffeq's continuous adjoint instead of reversing
        # the steps taken (include/xnwan.h, xw_ode_bwd mode bit 3); nabla_x u then only flows through the start value
        self.adjoint = bool(config.get('adjoint', False))
        self.alpha = float(config['alpha'])
        self.pollution = 1.0
        self.verify_structure = opt.verify_structure    # (_check_structure)
        self.packed_load = opt.packed_load     # list domains: load_groups_packed
        self.refill_variants = 8        # captured variants of a group's refill / diagnostic graph before further ones run eagerly
        self.verify_every = 16          # ~3 d + 1 callable evaluations per check: ~1 ms at d = 20, a fifth of an outer iteration
        sp = setup.get('shape_param', [-1, 1])
        lo, hi = (sp[0], sp[1]) if isinstance(sp, (list, tuple)) else (-sp, sp)
        self.structure = structure if structure is not None else Structure(funcs, self.d, lo, hi)
        if u_mod.blob is None or v_mod.blob is None:
            raise XnwanError('bind() the networks to the device before building the engine')
        # widths of the kernel instantiations the two networks run in (>= the configured widths: nets.Blob embeds a narrower
        # network exactly, zero-padded, in the next larger instantiation)
        (self.H, self.K), self.m = u_mod.kdims, config['u_layers']
        self.W, self.q = v_mod.kwidth, config['v_layers']
        # widths beyond the MFMA containers run on the generic path (csrc/xw_generic.hip): correct, deterministic, and two to three
        # orders of magnitude slower -- said once, loudly
        # the stepper family (kernels.stepper_family): the fused MFMA containers, the generic path or the tiled family
        # (csrc/xw_tiled.hip: any width up to 256 at the network's own widths, fixed grid; EngineOptions.tiled_stepper)
        # (solver 'explicit_adams': the tiled family at every width -- its only family)
        self.stepper = KN.stepper_family(config['u_hidden_dim'], config['u_hidden_hidden_dim'], self.m, opt.tiled_stepper, self.method)
        self.tiled = self.stepper == 'tiled'
        if self.method == KN.ADAMS and self.adjoint:
            from .nets import ADAMS_ADJOINT_REFUSED
            raise XnwanError(ADAMS_ADJOINT_REFUSED)
        if self.tiled:
            if (self.H, self.K) != (config['u_hidden_dim'], config['u_hidden_hidden_dim']):
                raise XnwanError('the tiled stepper family reads theta at the network\'s own widths; the module was bound at %s'
                                 % ((self.H, self.K),))
            if self.adjoint:
                raise XnwanError('adjoint=True (the continuous adjoint) is not served by the tiled stepper family (u_hidden_dim = %d, '
                                 'u_hidden_hidden_dim = %d, u_layers = %d: it reverses the steps taken; the continuous adjoint exists '
                                 'for the MFMA containers %s, u_layers <= %d)' % (self.H, self.K, self.m, KN.ODE_WIDTHS, KN.ODE_MAX_DEPTH))
            if self.dopri5 and self.dopri5_stepper != 'tiled':
                raise XnwanError("solver 'dopri5' is not served by the tiled stepper family (u_hidden_dim = %d, u_hidden_hidden_dim = %d, "
                                 "u_layers = %d): its field code is the generic path's, up to %s and u_layers %d; the tiled family runs "
                                 "the fixed-grid solvers %s -- unless EngineOptions.dopri5_stepper = 'tiled' (XW_DOPRI5_STEPPER) selects "
                                 "dopri5's implementation on that family" % (self.H, self.K, self.m, KN.GENERIC_ODE_MAX,
                                                                              KN.GENERIC_ODE_MAX_DEPTH, sorted(KN.METHODS)))
        # the test network's family (kernels.testnet_family): today's entry points (MFMA containers, generic path) or the tiled
        # family (csrc/xw_disc_tiled.hip: widths up to 256, depths up to 32, at the network's own width)
        self.testnet = getattr(v_mod, 'family', None) or KN.testnet_family(config['v_hidden_dim'], self.q)
        self.testnet_tiled = self.testnet == 'tiled'
        if self.testnet_tiled and self.W != config['v_hidden_dim']:
            raise XnwanError('the tiled test-network family reads phi at the network\'s own width; the module was bound at %d' % self.W)
        self.generic = (self.stepper == 'generic', not self.testnet_tiled and KN.disc_generic(self.W))
        if any(self.generic):
            import warnings
            which = ' and '.join(n_ for n_, g_ in zip(('u_theta (u_hidden_dim %d, u_hidden_hidden_dim %d, u_layers %d)' % (self.H, self.K, self.m),
                                                       'v_phi (v_hidden_dim %d)' % self.W), self.generic) if g_)
            warnings.warn('%s is outside the MFMA kernel instantiations %s (u_layers <= 10) / %s: running on the generic vector-ALU path, expect a step '
                          'rate lower by two to three orders of magnitude' % (which, KN.ODE_WIDTHS, KN.DISC_WIDTHS), RuntimeWarning, stacklevel=3)
        # the test network's input layer: spatial columns once per path (xw_disc_xproj) -- the MFMA widths, paths over a shared grid
        # XW_XPROJ_MIN_D: from which d on WITH the table formed at the head of the launch.  In that form the split wins in the sub-step
        # cycle from d ~ 45 on and not below, at 131072 points as at a million (profiles/r05_xproj.txt: headline d = 20 0.488 against
        # 0.473 ms per sub-step -- the small launch is one more dependent node on the critical chain --, d = 20 at 16384 x 64 3.41
        # against 3.38; d = 50 -1.3 %, BASELINE configs[2] -2.7 %, [3] -6.5 %).  Below it the table is only used where it is kept
        # across sub-steps and the head node is gone (xproj_cached, next paragraph).
        # (the tiled family hoists nothing: no table, at any width and depth)
        self.xproj_min_d = 1 << 30 if (self.generic[1] or self.testnet_tiled) else int(opt.xproj_min_d)
        if self.W > 64 and not self.generic[1] and not self.testnet_tiled:
            self.xproj_min_d = 0        # (the 128-wide container: 131 KB of Vh fragments leave no LDS for input-layer fragments -- always the table)
        # XW_XPROJ_CACHED: the table depends on phi and on the sample only, and inside an outer iteration every sub-step of a group sees
        # the same two -- so it is formed where the sample is loaded (load_group, refill_compact) and right behind the discriminator's
        # Adam, on the same queue, and a test-network launch whose table is still current (_xproj_state, decided outside captured code
        # like _v_fresh) has no head node.  Without the head node the hoisted main launch pays from xproj_cached_min_d on
        # (profiles/r16_xproj_cached.md).  A table that is not current -- phi written from outside, invalidate_test_net(), the other
        # groups of a sub-iteration over several groups, whose phi moves between their sub-steps -- is formed at the head as before.
        # Only the group a discriminator sub-step runs on gets the launch behind Adam: a captured graph would bake in the buffers of
        # whatever other groups were alive at capture time; their keys no longer match and they take the head launch.
        # The groups of a list domain loaded in one piece (load_groups_packed: 11-20 per sample, phi moving between their discriminator
        # sub-steps) keep no table below xproj_min_d: they run exactly as before.
        self.xproj_cached = bool(opt.xproj_cached) and self.xproj_min_d < (1 << 30)
        self.xproj_table_min_d = min(self.xproj_min_d, int(opt.xproj_cached_min_d)) if self.xproj_cached else self.xproj_min_d
        if self.generic[0] and self.adjoint:
            raise XnwanError('adjoint=True (the continuous adjoint) exists for the MFMA stepper instantiations %s only; u_hidden_dim = %d, '
                             'u_hidden_hidden_dim = %d run on the generic path, which reverses the steps taken (adjoint=False)'
                             % (KN.ODE_WIDTHS, self.H, self.K))
        self.theta, self.phi = u_mod.blob, v_mod.blob
        self.Pu, self.Pv = self.theta.data.numel(), self.phi.data.numel()
        z = lambda n: torch.zeros(n, dtype=F64, device=device)  # noqa: E731
        self.adam_u = dict(m=z(self.Pu), v=z(self.Pu), step=torch.zeros(1, dtype=torch.int64, device=device),
                           lag=torch.zeros(1, dtype=torch.int64, device=device))
        # Reference behaviour on the single-slice groups of the list domains (SURVEY A.4 / DESIGN 8 "Q8"), both on by default:
        #  * NeuralODE.forward returns [N,1] instead of [N,1,1] on a single-slice group at T0 (src/model.py:89-91) and the loss
        #    then broadcasts [N] against [N,1] into [N,N] tables over all PAIRS of paths (src/loss.py:65,70,79,84): reproduced
        #    in factorised O(N) form (load_group / xw_weak_partials pairwise).  XW_ELEMENTWISE_SINGLE_SLICE=1: the
        #    elementwise expressions instead (what the formulas mean; NOT what the reference computes).
        #  * such a group never integrates the ODE, so the field's parameters get no gradient; after zero_grad() (None on
        #    torch >= 2.0) Adam SKIPS them -- no moment decay, no step count -- until a group of the sub-iteration has taken an
        #    ODE step: the field range of the blob keeps its own step count (xw_adam lag / skip).
        self.pairwise_single_slice = opt.pairwise_single_slice
        self.adam_skips_untouched = opt.adam_skips_untouched
        self.eager_checked = 10 ** 12 if opt.always_check else 256
        self.field_range = (self.theta.slots[6][0], self.theta.slots[-2][0])      # Win .. Wo.b (nets._u_slots order)
        self._field_touched = False
        self.adam_v = dict(m=z(self.Pv), v=z(self.Pv), step=torch.zeros(1, dtype=torch.int64, device=device))
        self.grad_u, self.grad_v = z(self.Pu), z(self.Pv)   # the gradient Adam saw in the last sub-step
        # generator exchange buffer [sum of A slabs | sum of B slabs | scal]: ONE all-reduce per generator sub-step
        self.pack_u = z(2 * self.Pu + 16)
        self.scal = self.pack_u[2 * self.Pu:]
        # gradient carried from the previous groups of the same sub-iteration (list domains: the reference calls zero_grad()
        # once per sub-iteration but optimizer.step() after every group, src/training.py:127-138); None = off (one group)
        self.accum_u = self.accum_v = None
        self.use_streams = opt.use_streams   # independent kernel chains on side streams
        self.use_graphs = opt.use_graphs     # capture each sub-step into a HIP graph and replay it
        # opt-in: v, dv/dt, nabla_x v(t_0) of a group are reused while phi and the sample are unchanged (exact: the
        # reference recomputes identical values in every sub-step of an outer iteration).  Off by default.
        self.reuse_test_net = opt.reuse_test_net
        # both forwards store their layer inputs for their backwards (include/xnwan.h: XwOdeFwdJob.act, xw_disc_fwd act)
        self.keep_activations = opt.keep_activations
        # The test network's launch is persistent (grid-stride over point tiles) and at 2 blocks per CU it owns every SIMD's
        # register file: the stepper's waves, launched next to it, then wait until it drains.  Capping it below the
        # resident slots leaves SIMDs to the stepper chains.  With the kernel's ticket queues (tiles go to whichever wave is
        # free) the generator sub-step is flat between 9/16 and 11/16 of the slots (0.518 - 0.521 ms; 0.527 at 3/4, 0.533 at
        # 1/2); the static split needed exactly 3/4 (0.5225 ms, 0.58 either side).  Round 3 (leaner test network and stepper
        # forward): 10/16 -- cycle 1.546 / 1.541 / 1.554 / 1.557 ms at 9/16, 10/16, 11/16, 12/16.
        cus = torch.cuda.get_device_properties(device).multi_processor_count
        # Round 4: with the generator's sweeps A + boundary at lowered wave priority (prio_drop below) the test network keeps more of
        # the chip: generator sub-step 0.492 / 0.484 / 0.480 / 0.475 ms at 9, 10, 11, 12 sixteenths of the slots -- and 0.545 at 13 (a
        # cliff: the stepper's forward pass no longer finds SIMDs); 12/16.
        # (the 96- / 128-wide containers run one block per CU, the cap is clipped to all of them: 3/4 of the CUs measured the same with
        #  the wide stepper beside it and 6 % slower with the narrow one -- profiles/r06_width_step_rate.txt)
        self.v_blocks = int(opt.v_blocks) or (12 * 2 * cus) // 16
        # (discriminator sub-step: only the stepper forward and the x-only sweep run beside it, 33 us of SIMD time: 7/8 of the
        #  slots -- 0.615 ms against 0.638 at 3/4, 0.681 at 15/16, 0.735 at all of them; round 3: 13/16 and 14/16 equal
        #  (cycle 1.537 / 1.538 ms), 15/16 1.626; with the record stored through global instead of flat instructions the
        #  forward is 8 % shorter and the stepper's chain is what the sub-step waits for: 12/16 -- discriminator sub-step
        #  0.586 / 0.562 / 0.566 / 0.569 / 0.654 ms at 11..15 sixteenths, tools/sweep_caps.py)
        #  round 4: 0.583 / 0.566 / 0.563 / 0.566 ms at 11..14 sixteenths: 13/16)
        self.v_blocks_disc = int(opt.v_blocks_disc) or (13 * 2 * cus) // 16
        # Narrow tiles (csrc/xw_ode_n4.h, xw_ode_bwd mode bit 4): a 16-path tile of a sweep as four waves of 4 paths instead of one
        # (+ a partner) -- four times the instruction streams, each a shorter chain, at ~1.8 x the matrix-pipe time per path.
        # Used where a sweep runs with SIMDs to spare: sweep B of the generator sub-step (alone on the chip behind the test
        # network), as long as its waves still find a SIMD each.  XW_NARROW: 0 off, 1 auto (default), 2 wherever possible.
        self.narrow = str(opt.narrow)
        # wave-priority drops of the stepper launches that are not on a sub-step's critical path (include/xnwan.h: xw_ode_bwd mode
        # bits 5..6, XwOdeFwdJob.prio_drop): A = the generator's sweeps A + boundary, X = the discriminator's x-only sweep,
        # F = the discriminator's forward pass, G = the generator's.  A = 3 puts sweeps A + boundary at the test network's own
        # priority (0): 0.4764 against 0.4838 ms per sub-step at 2 (tools/cap_sweep.sh, three alternating runs each; found at the end
        # of round 4: the first sweep stopped at 2); G = 1..2 and X, F = 1 are within the noise of that, G = 3 loses 7 %.
        # At larger d the test network's launch is longer relative to the stepper's chains (its input layer and the fused
        # nabla_x v grow with d, the stepper's x-projection is hoisted) and sweeps that never get ahead of it end AFTER sweep B:
        # tools/ab_cfg_prio.sh, priority 1 against 0 -- d = 20: -1.4 % / -1.1 % at 4096 / 8192 paths, equal at 2048; d = 50: equal
        # at 2048 x 64, +0.8 % at 16384 x 64; d = 100: +1.2 % at 8192, +1.3 % at 65536.  Default: 3 up to d = 32, 2 above.
        # The sub-step graphs' four chains are laid out for the HIP runtime's default of FOUR hardware queues: with 5, 6 or 8
        # (GPU_MAX_HW_QUEUES) the headline sub-step takes 0.69 instead of 0.47 ms (tools/hwq.sh; 2 and 3 are as good as 4).
        if opt.hw_queues > 4:
            import warnings
            warnings.warn('GPU_MAX_HW_QUEUES=%s: the sub-step schedule is tuned for the runtime default of 4 hardware queues and '
                          'measures ~45 %% slower with more' % opt.hw_queues, RuntimeWarning, stacklevel=2)
        self.early_slab_sum = opt.early_slab_sum
        # groups of at most this many 16-path tiles (interior + boundary) take the compact schedule of _gen_front_compact (0: never).
        # tools/shard_streams.sh, ms per sub-step wide / compact: 256 paths (+ 256 boundary paths) 0.2489 / 0.2183, 512 0.2609 / 0.2244,
        # 1024 0.2829 / 0.2487, 1536 0.3190 / 0.3108, 2048 0.3490 / 0.3432, 2560 0.3931 / 0.3791, 3072 0.4173 / 0.4272, 4096 0.4698 / 0.4919
        self.compact_tiles = int(opt.compact_tiles)
        # one GPU: the generator's interior sweeps A and B as ONE sweep over A + (2/I) B (_gen_front_merged); off = the two-sweep
        # schedules below for every group (XW_MERGED_SWEEP=0: the same build measured both ways)
        self.merged_sweep = bool(opt.merged_sweep)
        self.prio_drop = {'A': int(opt.prio_drop_A) if opt.prio_drop_A is not None else (3 if self.d <= 32 else 2),
                          'X': int(opt.prio_drop_X), 'F': int(opt.prio_drop_F), 'G': int(opt.prio_drop_G)}
        self.use_runner = opt.use_runner      # one C call per eager group sub-step (xw_substep_*)
        if self.dopri5:
            self.use_graphs = self.use_streams = self.use_runner = self.keep_activations = False
        if self.tiled:
            # the group runner (xw_substep_*) is fused fixed-family C; the tiled sweeps recompute from Y (no activation store) and
            # have no narrow tiles.  Graphs and streams stay on.
            self.use_runner = self.keep_activations = False
            self.narrow = '0'
        if self.testnet_tiled:
            # the group runner (xw_substep_*) calls the MFMA entry points directly; the test network keeps its record (vact)
            self.use_runner = False
        # Measured (profiles/r04_shard_sweep.md): forward and the sweep without weight gradients gain on shards up to ~2048
        # paths (0.302 -> 0.272 ms per sub-step at 512 paths, 0.332 -> 0.294 at 1024, 0.375 -> 0.367 at 2048); the narrow sweep
        # WITH weight gradients only ties the two-wave duo sweep (88 against 83 us alone) and is left to XW_NARROW_SET=fxp; at
        # the headline size everything narrow LOSES (0.502 -> 0.586 ms): those phases are bound by the sum of SIMD time.
        self.narrow_set = str(opt.narrow_set)
        self.narrow_tiles = {'f': 192, 'x': 128, 'p': 64}    # largest launch (16-path tiles, all its jobs) that still gains
        if opt.narrow_tiles:                                 # (measurements: "f:x:p")
            self.narrow_tiles = dict(zip('fxp', (int(v_) for v_ in str(opt.narrow_tiles).split(':'))))
        # ... and for a launch that has the chip to itself (tools/kernel_times.py at 256 / 512 tiles, profiles/r06_kernel_times.txt)
        self.narrow_tiles_alone = dict(zip('fxp', (int(v_) for v_ in str(opt.narrow_tiles_alone).split(':'))))
        for k_ in 'fxp':
            self.narrow_tiles_alone[k_] = max(self.narrow_tiles_alone[k_], self.narrow_tiles[k_])
        self.simds = 4 * cus
        self._phi_version = 0
        self.streams, self._cap = _device_streams(device)
        # several GPUs on RCCL: the exchanges are device-side calls on the current stream (dist.World.capturable), so a
        # sub-step and its exchange(s) are captured into ONE HIP graph instead of graph / host call / graph
        self.capture_exchange = (world is not None and getattr(world, 'capturable', False)
                                 and opt.capture_exchange)
        if self.capture_exchange:
            world.all_reduce(self.scal)           # (zeros) first use outside any capture: RCCL sets up its channels here

    # ------------------------------------------------------------------------------------------------------------
    # building blocks
    # ------------------------------------------------------------------------------------------------------------
    def _side(self, i, *events):
        """context: run on side stream i after `events` (falls back to the current stream when streams are off)"""
        if not self.use_streams:
            return _NOSTREAM                      # one stream: program order is the dependency (no contexts, no events)
        st = self.streams[i]
        for ev in events:
            if ev is not None:
                st.wait_event(ev)
        return torch.cuda.stream(st)

    def _mark(self):
        return torch.cuda.current_stream().record_event() if self.use_streams else None

    def _join(self, *events):
        if self.use_streams:
            cur = torch.cuda.current_stream()
            for ev in events:
                if ev is not None:
                    cur.wait_event(ev)

    def _launch_test_net_here(self, G, blocks=None):
        """test network on the CURRENT stream (the sub-step's critical chain): v, dv/dt at all points; nabla_x v at the first
        time index rides along in the same launch (fused reverse chain); optionally the record of layer inputs for the
        backward (decided in _v_fresh, outside the captured code)"""
        ph, blocks = self.phi.data, blocks or self.v_blocks
        act = G.vact if getattr(G, 'vact_valid', False) else None
        if G.tpp is not None:
            KN.disc_fwd(G.xvT_pts, None, ph, self.W, self.q, tpp=G.tpp, v=G.v.view(1, -1), vt=G.vt.view(1, -1),
                        gxv=G.gxv, gtv=G.gtv, ngrad=G.N, max_blocks=blocks, act=act)
        else:
            # (the input layer's spatial columns do not move along a vertical path: applied once per path by a small launch in
            #  front, csrc/xw_disc_fwd.hip k_disc_xproj -- the main launch then loads its row of that table instead of x)
            #  -- unless the group's table is still that of this phi and this sample: _xproj_state)
            xp = None
            if 'xproj' in G._lazy:
                xp = G.xproj if getattr(G, 'xproj_cur', False) else KN.disc_xproj(G.xvT, ph, self.W, out=G.xproj)
            KN.disc_fwd(G.xvT, G.t, ph, self.W, self.q, v=G.v, vt=G.vt, gxv=G.gxv, gtv=G.gtv, ngrad=G.N,
                        max_blocks=blocks, act=act, xproj=xp)

    def _reaction(self, G):
        """c(u, t, x): linear fast path, or the user's callable differentiated by autograd (not graph-capturable)"""
        ck = self.structure.c_kappa
        if ck is None and G.pair_i:
            # single-slice group at T0: the reference hands its callable u as [N, 1] there (src/model.py:89-91), not [N, 1, 1], and takes
            # `c.squeeze() * u.squeeze() * phi.squeeze()` summed over ALL its entries (src/loss.py:70).  A callable that mixes u with a
            # slice of X that kept its last axis ([N, 1, 1]) thereby returns the TABLE c[m, n] = c(u_n, x_m): per path n the term is
            # sum_m c[m, n] u_n phi_n = N mean_m c[m, n] u_n phi_n -- the N is the one every term of such a group carries (s3_scale)
            N = G.N
            ul = G.u.t().detach().requires_grad_(True)                           # [N, 1]
            with torch.enable_grad():
                c = self.funcs['c'](G.X, ul)
                c = c.reshape(N, N) if c.numel() == N * N and N > 1 else c.reshape(-1)
                if c.dim() == 2:
                    if getattr(G, 'sharded', False):
                        raise XnwanError('func_c returns a table over all pairs of paths on a single-slice group (it mixes u [N, 1] with a slice of X that '
                                         'kept its last axis): that needs every path of the group on one rank -- run such groups replicated '
                                         '(XW_REPLICATE_BELOW >= their size) or on one GPU')
                    c = c.mean(0)
                elif c.numel() != N:
                    raise XnwanError('func_c on a single-slice group returned %d values for %d paths' % (c.numel(), N))
                cp = torch.autograd.grad(c.sum(), ul)[0] if c.requires_grad else torch.zeros_like(ul)
            if G.c is None:
                G.c, G.cp = torch.empty_like(G.u), torch.empty_like(G.u)
            G.c.copy_(c.detach().reshape(1, N))
            G.cp.copy_(cp.detach().reshape(1, N))
            ck = 0.0
        elif ck is None:
            ul = G.u.t().unsqueeze(2).detach().requires_grad_(True)
            with torch.enable_grad():
                c = self.funcs['c'](G.X, ul)
                cp = torch.autograd.grad(c.sum(), ul)[0] if c.requires_grad else torch.zeros_like(ul)
            if G.c is None:
                G.c, G.cp = torch.empty_like(G.u), torch.empty_like(G.u)     # (persistent: captured graphs keep reading them)
            G.c.copy_(c.detach().squeeze(2).t())
            G.cp.copy_(cp.detach().squeeze(2).t())
            ck = 0.0
        G.ck = ck

    # ------------------------------------------------------------------------------------------------------------
    # one C-ABI call per group sub-step (xw_substep_gen / xw_substep_disc, csrc/xw_substep.hip) for the groups that run
    # eagerly -- the 11-20 groups per sample of the list domains, new shapes every sample: ~15 launches per group and
    # sub-step issued from Python one by one cost more host time than the GPU needs to run them
    # ------------------------------------------------------------------------------------------------------------
    def _runner_state(self):
        """XwSolverState of this engine (pointers to buffers that live as long as the engine)"""
        from ._lib import XwSolverState
        st = getattr(self, '_xw_state', None)
        if st is None:
            st = self._xw_state = XwSolverState()
            st.method, st.H, st.K, st.m, st.W, st.q, st.Pu, st.Pv = self.method, self.H, self.K, self.m, self.W, self.q, self.Pu, self.Pv
            st.adjoint = 1 if self.adjoint else 0
            st.lag_lo, st.lag_hi = self.field_range
            st.beta1, st.beta2, st.eps = 0.9, 0.999, 1e-8
            st.theta, st.phi, st.scal = self.theta.data.data_ptr(), self.phi.data.data_ptr(), self.scal.data_ptr()
            st.grad_u, st.grad_v = self.grad_u.data_ptr(), self.grad_v.data_ptr()
            st.m_u, st.v_u, st.m_v, st.v_v = (self.adam_u['m'].data_ptr(), self.adam_u['v'].data_ptr(), self.adam_v['m'].data_ptr(),
                                              self.adam_v['v'].data_ptr())
            st.step_u, st.step_v, st.lag_u = self.adam_u['step'].data_ptr(), self.adam_v['step'].data_ptr(), self.adam_u['lag'].data_ptr()
            st.exchange = st.exchange_ctx = st.pack_u = None
            if self.world is not None:
                st.pack_u = self.pack_u.data_ptr()
                if self.world.comm is not None:            # RCCL: the library's own entry point, enqueued on the stream like the kernels
                    from ._lib import lib
                    import ctypes
                    st.exchange = ctypes.cast(lib.xw_allreduce, ctypes.c_void_p).value
                    st.exchange_ctx = self.world.comm.value if hasattr(self.world.comm, 'value') else self.world.comm
                else:                                      # rehearsal (gloo): a host-side stand-in with the same contract
                    self._exchange_cb = self._host_exchange()
                    st.exchange = ctypes_addr(self._exchange_cb)
        st.v_blocks, st.v_blocks_disc = self.v_blocks, self.v_blocks_disc
        st.merged_sweep = int(self.merged_sweep)
        st.alpha, st.pollution = float(self.alpha), float(self.pollution)
        st.lr_u, st.lr_v = float(self.config['u_rate']), float(self.config['v_rate'])
        return st

    def _host_exchange(self):
        """XwSolverState.exchange without RCCL (the `gloo` rehearsal: several ranks on one GPU, tests): the same contract as
        xw_allreduce -- in-place float64 sum of buf[count] over the ranks, in stream order -- through torch.distributed with the
        buffer staged on the host.  The runner only ever passes the engine's own exchange buffers."""
        from ._lib import EXCHANGE_FN
        bufs = {t.data_ptr(): t for t in (self.pack_u, self.scal, self.grad_v)}

        def exchange(buf, count, _ctx, _stream):
            try:
                self.world.all_reduce(bufs[buf][:count])
                return 0
            except BaseException as e:          # (an exception cannot cross the C frames: kept for the caller, reported as XW_E_COMM)
                self._exchange_error = e
                return -4
        return EXCHANGE_FN(exchange)

    def _runner_group(self, G):
        """XwGroup of a loaded group: pointers once per allocation, the per-sample scalars every time"""
        from ._lib import XwGroup
        xg = getattr(G, '_xw_group', None)
        if xg is None:
            xg = G._xw_group = XwGroup()
            p = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
            xg.N, xg.Nb, xg.L, xg.Lb, xg.d = G.N, G.Nb, G.L, G.Lb, self.d
            xg.same_grid, xg.w_per_point, xg.amode = int(bool(G.same_grid)), int(G.w.dim() == 2), int(G.amode)
            xg.ns_u, xg.ns_b = G.ns_u, G.ns_b
            for k in ('xT', 'xvT', 'xbT', 't', 'tb', 'tpp', 'xvT_pts', 'start', 'start_b', 'h', 'href', 'f', 'g', 'w', 'wt', 'w0', 'ghT',
                      'gwx0T', 'A0', 'B0', 'u', 'Y', 'act', 'act_b', 'v', 'vt', 'gxv', 'gtv', 'gx', 'gs', 'vbar', 's3x', 'vact',
                      'xproj', 'slabA', 'slabB', 'slab_v', 'work_i', 'work_b', 'ub', 'Yb'):
                setattr(xg, k, G.ptr(k))         # (addresses only: the work buffers' tensor views are made when Python reads them)
            nar = lambda jobs, **kw: self._narrow_ok(jobs, **kw)  # noqa: E731
            ji, jb = self._job(G, 'i'), (self._job(G, 'b') if G.Nb else None)
            joint = G.Nb and G.same_grid
            # (bit 2: the runner launches sweep A, the boundary sweep on the same grid and sweep B as ONE launch -- the tile count
            #  that decides is that launch's, as in _gen_front_compact; bit 4: the merged form's launch {interior kind 3, boundary})
            bits = [nar([ji] + ([jb] if joint else []), alone=False, forward=True),
                    bool(jb) and nar([jb], alone=False, forward=True),
                    nar([ji] + ([jb] if joint else []) + [ji], alone=False),
                    bool(jb) and nar([jb], alone=False),
                    bool(joint) and nar([ji, jb], alone=False),
                    nar([ji], alone=False, params=False),
                    nar([ji], alone=False, forward=True),
                    nar([ji], alone=False, params=False)]
            xg.narrow = sum(1 << i for i, b in enumerate(bits) if b)
        xg.sharded = int(bool(getattr(G, 'sharded', False)))
        xg.xproj_current = (2 if getattr(G, 'xproj_cur', False) else 1) if self._xproj_held(G) else 0
        xg.pair_i, xg.pair_b = int(bool(G.pair_i)), int(bool(G.pair_b))
        xg.Vol, xg.Nglob, xg.Nbglob, xg.s3_scale = float(G.Vol), float(G.Nglob), float(G.Nbglob), float(G.s3_scale)
        xg.init_off, xg.bdry_off, xg.ckappa = float(G.init_off), float(G.bdry_off), float(self.structure.c_kappa)
        xg.href = 0 if G.href is None else G.href.data_ptr()
        xg.c = xg.cp = 0
        return xg

    def _runner_ok(self, G):
        return (self.use_runner and self.structure.c_kappa is not None and G.c is None and not getattr(G, 'persistent', True))

    def _world_of(self, G):
        """the ranks that hold shares of G: None when the whole group is here (one process, or a group every rank computes in
        full -- dist.World.replicated -- with the single-process arithmetic and no exchange)"""
        return self.world if getattr(G, 'sharded', self.world is not None) else None

    def _field_seen(self, G):
        """has a group of this sub-iteration integrated the ODE yet?  (no: the field's parameters have no gradient, Adam skips
        them -- Engine.__init__.)  From facts every rank shares: `has_bdry` is the GROUP's, not this rank's possibly empty share"""
        touched = G.L > 1 or (getattr(G, 'has_bdry', G.Nb > 0) and G.Lb > 1)
        self._field_touched = touched or (self.accum_u is not None and self._field_touched)
        return self._field_touched

    def _narrow_ok(self, jobs, alone, forward=False, params=True):
        """narrow tiles (csrc/xw_ode_n4.h) for this stepper launch?  XW_NARROW: 0 never, 1 by size (default), 2 wherever the
        kernels exist; XW_NARROW_SET: which launches may (f forward, x sweeps without weight gradients, p sweeps with them)"""
        kind = 'f' if forward else ('p' if params else 'x')
        if self.narrow == '0' or kind not in self.narrow_set:
            return False
        if not forward and (self.adjoint or self.method > 1 or any(j.get('act') is None for j in jobs)):
            return False
        if self.narrow == '2':
            return True
        tiles = sum((j['xT'].shape[1] + 15) // 16 for j in jobs)
        # `alone`: nothing else runs beside this launch (the test network is reused / this is a lone evaluation) -- the narrow
        # forms then gain up to larger launches (narrow_tiles_alone), they need SIMDs to spare, not a short chain only
        return tiles <= (self.narrow_tiles_alone if alone else self.narrow_tiles)[kind]

    def _job(self, G, which, ubar=None, gslab=None, want_x=False):
        if which == 'i':
            j = dict(xT=G.xT, start=G.start, u=G.u, Y=G.Y, act=G.act, ubar=ubar, gslab=gslab)
            if want_x:
                j.update(gx=G.gx, gs=G.gs)
        else:
            j = dict(xT=G.xbT, start=G.start_b, u=G.ub, Y=G.Yb, act=G.act_b, ubar=ubar, gslab=gslab)
        return j

    # The residual forms of the generator's sweeps (kernels._set_res), each once: what csrc/xw_substep.hip restates for the runner's groups
    def _res_init(self, G):      # cotangent A: pollution + the initial-value penalty at t_0
        # (pairwise group: the initial penalty is the mean over all PAIRS (u_n - h_m)^2, whose u-gradient is 2 (u_n - mean h) / N)
        return dict(u=G.u, ref=G.href if G.pair_i else G.h, coef=2.0 * self.alpha / G.Nglob, base=self.pollution, first_only=True)

    def _res_bdry(self, G):      # the boundary penalty's cotangent (only for a group with boundary paths: Nbglob Lb > 0)
        return dict(u=G.ub, ref=G.g, coef=2.0 * self.alpha / (G.Nbglob * G.Lb), base=0.0, first_only=False)

    def _res_weak(self, G):      # cotangent B = dI/du, a pointwise product of what the two forward passes wrote (kind 2)
        return dict(u=G.u, ref=G.v, coef=G.Vol / G.Nglob / G.L * G.s3_scale, base=G.Vol / G.Nglob, weak=dict(w=G.w, c=G.c, cp=G.cp, ckappa=G.ck))

    def _res_merged(self, G):    # kind 3, A + (2 / I) B: B with A's ref, coef and base (_merged_ok: no pairwise group, ref = h) and I = scal[0]
        return dict(self._res_weak(G), merged=dict(self._res_init(G), scal=self.scal))

    def _contract(self, G, adam_state=None, with_bdry=False):
        """I, sum v^2, SSE_init from u, v, dv/dt and the two helper-backward gradients (src/loss.py:46-76).
        Single GPU: the sums are global, so the same launch also forms the loss values and advances the optimiser's
        counter (`adam_state`); with several GPUs that is done by KN.losses after the all-reduce."""
        fin = None
        if self._world_of(G) is None and adam_state is not None:
            fin = dict(Lb=G.Lb, Nbglob=G.Nbglob, alpha=self.alpha, step=adam_state['step'], init_off=G.init_off, bdry_off=G.bdry_off)
        pair = dict(href=G.href, s3_scale=G.s3_scale) if G.pair_i else None
        # generator sub-step: the boundary penalty's sum of squares (a loss value; the sweeps form its cotangent themselves) rides along
        bdry = dict(ub=G.ub, g=G.g) if (with_bdry and G.Nb) else None
        if G.A0 is None and G.B0 is None:
            KN.weak_partials(G.u, G.v, G.vt, G.w, G.f, G.h, G.Vol, G.Nglob, self.scal, G.work_i, c=G.c, ckappa=G.ck, wt=G.wt,
                             contract=dict(gx=G.gx, gs=G.gs, ghT=G.ghT, gxv=G.gxv, w0=G.w0, gwx0T=G.gwx0T), finalize=fin, pair=pair,
                             bdry=bdry)
            return
        # general a_ij / b_i: the l = 0 contraction as one streaming kernel over the tabulated slice (graph-capturable)
        KN.weak_contract_general(G.A0, G.amode, G.B0, G.gx, G.gs, G.ghT, G.gxv, G.w0, G.gwx0T, G.v[0], G.s3x)
        KN.weak_partials(G.u, G.v, G.vt, G.w, G.f, G.h, G.Vol, G.Nglob, self.scal, G.work_i, s3x=G.s3x, c=G.c, ckappa=G.ck,
                         wt=G.wt, finalize=fin, pair=pair, bdry=bdry)

    # ------------------------------------------------------------------------------------------------------------
    # generator sub-step (src/training.py:127-138)
    # ------------------------------------------------------------------------------------------------------------
    def _gen_all(self, G):
        """single GPU: the whole generator sub-step is one captured graph"""
        self._gen_front(G)
        self._gen_back(G)

    def _gen_front(self, G):
        """everything up to (not including) the exchange: leaves slabA, slabB and scal[0..3] complete (the merged form,
        _gen_front_merged: slabA and scal[0..3] only -- slabB is not written, G.merged tells _gen_back).
        Kernel chains of the wide schedule:
                        main  test network v, dv/dt and (fused) nabla_x v(t_0) -> cotangent B = dI/du -> parameter
                               sweep B -> [join] -> I, sum v^2, SSE, loss values            (the critical path: one stream,
                               dependent launches of one stream follow each other without the ~10 us cross-queue hop)
                        side 1 u-forward (interior + boundary, one launch) -> boundary residual -> cotangent A
                               -> parameter sweeps {interior/A, boundary} (one launch; sweep A also returns nabla_x u:
                               same adjoint as the helper backward)"""
        th = self.theta.data
        M = (self.method, self.H, self.K, self.m)
        e0 = self._mark()
        fused_x = self.pollution == 1.0 and not self.adjoint
        joint = G.Nb and G.same_grid           # boundary paths on the interior's time grid: one launch for both
        e_x = None
        G.merged = self._merged_ok(G, fused_x, joint)
        if G.merged:
            return self._gen_front_merged(G)
        if self._compact(G, fused_x, joint):
            return self._gen_front_compact(G)
        if not getattr(G, 'skip_v', False):
            self._launch_test_net_here(G)                        # enqueued first: its blocks must be resident before the
        with self._side(1, e0):                                  # stepper's waves spread over the CUs
            fwd = [self._job(G, 'i')] + ([self._job(G, 'b')] if joint else [])
            self._ode_fwd_multi(fwd, G.t, th, *M, zero16=self.scal, narrow=self._narrow_ok(fwd, alone=False, forward=True),
                             prio_drop=self.prio_drop['G'])
            if G.Nb and not joint:
                fwd_b = [self._job(G, 'b')]
                self._ode_fwd_multi(fwd_b, G.tb, th, *M, narrow=self._narrow_ok(fwd_b, alone=False, forward=True))
            self._reaction(G)
            e_f = self._mark()
            # Cotangent A (pollution + the initial-value penalty at t_0) and the boundary cotangent are residuals of what
            # the forward pass just wrote: the sweeps form them on the fly (XwOdeBwdJob.res_*) and start right behind the
            # forward pass -- the boundary sum of squares (a loss value, not an input of any sweep) runs beside them.  One
            # launch and two [L, N] buffers fewer per sub-step; the cycle does not change (1885 steps/s either way): the
            # sweeps start 26 us earlier, next to the test network, whose launch then lasts that much longer -- the first
            # phase of the sub-step is bound by SIMD time, not by this chain.
            e_b = None       # (the boundary sum of squares, a loss value only, is formed by the reduction at the end: _contract(with_bdry))
            # With the reference's pollution (cotangent A = ones + the initial-value term at t_0) sweep A and the helper
            # backward u.backward(ones) are the same adjoint: one launch returns the parameter gradient of A and nabla_x u.
            if not fused_x:
                with self._side(2, e_f):
                    sweep_x = [self._job(G, 'i', want_x=True)]
                    self._ode_bwd_multi(sweep_x, G.t, th, *M, want_x=True, want_params=False, adjoint=self.adjoint,
                                     narrow=self._narrow_ok(sweep_x, alone=False, params=False))
                    e_x = self._mark()
            sweeps = [dict(self._job(G, 'i', None, G.slabA[:G.ns_u], want_x=fused_x), res=self._res_init(G))]
            if joint:
                sweeps.append(dict(self._job(G, 'b', None, G.slabA[G.ns_u:]), res=self._res_bdry(G)))
            self._ode_bwd_multi(sweeps, G.t, th, *M, want_x=fused_x, want_params=True, x_cot_ones=fused_x, adjoint=self.adjoint,
                             narrow=self._narrow_ok(sweeps, alone=False), prio_drop=self.prio_drop['A'])
            if G.Nb and not joint:
                sweep_b = [dict(self._job(G, 'b', None, G.slabA[G.ns_u:]), res=self._res_bdry(G))]
                self._ode_bwd_multi(sweep_b, G.tb, th, *M, want_x=False, want_params=True, adjoint=self.adjoint,
                                 narrow=self._narrow_ok(sweep_b, alone=False))
            e_A = self._mark()
            # The slabs of sweeps A + boundary are summed HERE, beside the tail of sweep B, so that the update at the end of the sub-step
            # only has sweep B's slabs left to read (k_slab_sum is the A half of k_adam's own summation tree: the same bits).
            G.sumA_ready = self.early_slab_sum and self._world_of(G) is None and self.accum_u is None and self.use_streams
            e_S = None
            if G.sumA_ready:
                if getattr(G, 'sumA', None) is None:
                    G.sumA = torch.empty(self.Pu, dtype=F64, device=self.dev)
                KN.slab_sum(G.slabA, out=G.sumA)
                e_S = self._mark()
        e_v = self._mark()
        self._join(e_f)
        # cotangent B = dI/du is a pointwise product of what the two forward passes wrote: sweep B forms it on the fly too
        # (XwOdeBwdJob.res_first_only = 2) and starts right behind the test network: one launch fewer on the critical chain
        # test network -> sweep B -> Adam (0.5063 -> 0.5034 ms per generator sub-step in the same run)
        sweep_B = [dict(self._job(G, 'i', None, G.slabB), res=self._res_weak(G))]
        self._ode_bwd_multi(sweep_B, G.t, th, *M, want_x=False, want_params=True, adjoint=self.adjoint,
                         narrow=self._narrow_ok(sweep_B, alone=True))
        # the reduction needs nabla_x u (sweep A) and v, not sweep B: it runs behind sweep A on the side stream, next to
        # the tail of sweep B, instead of after it
        with self._side(3, e_A, e_v, *[e for e in (e_x, e_b) if e is not None]):   # (re-entering side 1 here crashes hipStreamEndCapture)
            self._contract(G, self.adam_u, with_bdry=True)       # -> scal[0..3], loss values
            e_C = self._mark()
        self._join(e_C, e_S)

    def _compact(self, G, fused_x, joint):
        """small groups (shards of a strong-scaling job, small problems): the sub-step is a chain of dependent launches whose
        every cross-queue dependency edge costs ~12 us -- the compact schedule below has one instead of three"""
        tiles = (G.N + 15) // 16 + ((G.Nb + 15) // 16 if G.Nb else 0)
        if not (self.compact_tiles > 0 and self.use_streams and fused_x and joint):
            return False
        # ... and ANY group whose test network is not evaluated in this sub-step (v, dv/dt, nabla_x v(t_0) reused while phi and the
        # sample are unchanged: the second generator sub-iteration of train()): nothing holds sweep B back, the chip is empty, and
        # the three sweep jobs in one launch take 146 us where sweeps A + boundary (139) and B (94) followed each other -- as branches
        # of the wide graph they land on one hardware queue behind the reduction (profiles/r06_train_timeline.txt)
        return tiles <= self.compact_tiles or bool(getattr(G, 'skip_v', False))

    def _gen_front_compact(self, G):
        """_gen_front for a group that leaves the chip mostly idle: test network (main) || forward pass (side 1), then ON THE MAIN
        STREAM one launch with all three sweep jobs (A with nabla_x u, boundary, B), the reduction and (in _gen_back) the update --
        same kernels, same arguments, same results as the wide schedule; dependent launches of one stream follow each other without
        the cross-queue hop."""
        th = self.theta.data
        M = (self.method, self.H, self.K, self.m)
        e0 = self._mark()
        if not getattr(G, 'skip_v', False):
            self._launch_test_net_here(G)
        with self._side(1, e0):
            fwd = [self._job(G, 'i'), self._job(G, 'b')]
            lone = bool(getattr(G, 'skip_v', False))
            self._ode_fwd_multi(fwd, G.t, th, *M, zero16=self.scal, narrow=self._narrow_ok(fwd, alone=lone, forward=True),
                             prio_drop=self.prio_drop['G'])
            self._reaction(G)
            e_f = self._mark()
        self._join(e_f)
        sweeps = [dict(self._job(G, 'i', None, G.slabA[:G.ns_u], want_x=True), res=self._res_init(G)),
                  dict(self._job(G, 'b', None, G.slabA[G.ns_u:]), res=self._res_bdry(G)),
                  dict(self._job(G, 'i', None, G.slabB), res=self._res_weak(G))]
        self._ode_bwd_multi(sweeps, G.t, th, *M, want_x=True, want_params=True, x_cot_ones=True, adjoint=self.adjoint,
                         narrow=self._narrow_ok(sweeps, alone=bool(getattr(G, 'skip_v', False))))
        G.sumA_ready = False
        self._contract(G, self.adam_u, with_bdry=True)

    def _merged_ok(self, G, fused_x, joint):
        """does this group's generator sub-step take the merged form?  One GPU, no carried gradient, the fused helper backward,
        boundary paths on the interior's grid, no pairwise sums, a = identity and b = 0 (the same rule as xw_substep_gen's; every
        stepper family forms the merged cotangent, XwOdeBwdJob.res_first_only == 3)"""
        return bool(self.merged_sweep and self._world_of(G) is None and self.accum_u is None and fused_x and joint
                    and not (G.pair_i or G.pair_b) and G.A0 is None and G.B0 is None)

    def _gen_front_merged(self, G):
        """_gen_front with ONE interior parameter sweep.  The update needs J^T A + (2/I) J^T B = J^T (A + (2/I) B): once I is on the
        device the sweep forms the summed cotangent itself (kind 3) and the interior paths are swept once with weight gradients,
        not twice.  I needs nabla_x u(t_0): an x-only sweep (one wave per tile, no partner wave, no slabs) delivers it beside the
        test network, as in the discriminator sub-step.
        Kernel chains:  main   test network -> [join] -> I, sum v^2, SSE, loss values -> sweeps {interior kind 3, boundary} (one
                               launch, one slab set) -> Adam (in _gen_back)
                        side 1 u-forward (interior + boundary, full store) -> x-only sweep from the store
        One cross-queue edge; the same launches in the same order whether captured, eager or issued by xw_substep_gen.
        Tile layout: every launch here asks _narrow_ok with alone=False, also when the test network is reused (skip_v) and the
        launches do have the chip to themselves -- the `narrow_tiles_alone` thresholds, which _gen_front_compact applies in that
        case, do NOT apply under the merged form.  The runner holds one precomputed layout bit per launch (XwGroup.narrow), and the
        two layouts sum in different orders, so a second set of thresholds would have to reach both to keep reuse on / off and
        runner / launch-by-launch bit-identical; not done, and not measured (at the headline only the x-only sweep, 256 tiles,
        would change layout)."""
        th = self.theta.data
        M = (self.method, self.H, self.K, self.m)
        lone = bool(getattr(G, 'skip_v', False))      # (only decides whether the test network is evaluated)
        e0 = self._mark()
        if not lone:
            self._launch_test_net_here(G)
        with self._side(1, e0):
            fwd = [self._job(G, 'i'), self._job(G, 'b')]
            self._ode_fwd_multi(fwd, G.t, th, *M, zero16=self.scal, narrow=self._narrow_ok(fwd, alone=False, forward=True),
                             prio_drop=self.prio_drop['G'])
            self._reaction(G)
            sweep_x = [self._job(G, 'i', want_x=True)]
            self._ode_bwd_multi(sweep_x, G.t, th, *M, want_x=True, want_params=False,
                             narrow=self._narrow_ok(sweep_x, alone=False, params=False))
            e_x = self._mark()
        self._join(e_x)
        self._contract(G, self.adam_u, with_bdry=True)           # -> scal[0] = I, loss values, the optimiser's counter
        sweeps = [dict(self._job(G, 'i', None, G.slabA[:G.ns_u]), res=self._res_merged(G)),
                  dict(self._job(G, 'b', None, G.slabA[G.ns_u:]), res=self._res_bdry(G))]
        self._ode_bwd_multi(sweeps, G.t, th, *M, want_x=False, want_params=True, narrow=self._narrow_ok(sweeps, alone=False))
        G.sumA_ready = False

    def begin_substep(self, which, accumulate):
        """start of a generator ('u') / discriminator ('v') sub-iteration over several groups: zero the carried gradient"""
        name, P = ('accum_u', self.Pu) if which == 'u' else ('accum_v', self.Pv)
        if which == 'u':
            self._field_touched = False
        if not accumulate:
            setattr(self, name, None)
        elif getattr(self, name) is None:
            setattr(self, name, torch.zeros(P, dtype=F64, device=self.dev))
        else:
            getattr(self, name).zero_()

    def _gen_back(self, G):
        lr, st = self.config['u_rate'], self.adam_u
        acc = self.accum_u
        world = self._world_of(G)
        lag = dict(lag=st['lag'], lag_range=self.field_range, skip=self.adam_skips_untouched and not self._field_seen(G))
        if world is not None:     # (the whole group here: loss values and counter were done by the reduction launch, _contract)
            if G.pair_i:
                KN.pair_fold(self.scal, G.Vol, G.Nglob)
            KN.losses(self.scal, G.L, G.Lb, G.Vol, G.Nglob, G.Nbglob, self.alpha, step=st['step'], init_off=G.init_off,
                      bdry_off=G.bdry_off)
        if world is None and getattr(G, 'merged', False):
            # one slab set, weighted inside the sweep: no scal, coefB = 1
            KN.adam(self.theta.data, G.slabA, st['m'], st['v'], st['step'], lr, gsum_out=self.grad_u, bump_step=-1, **lag)
        elif world is None and getattr(G, 'sumA_ready', False) and acc is None:
            KN.adam(self.theta.data, None, st['m'], st['v'], st['step'], lr, gslabB=G.slabB, scal=self.scal,
                    gextraA=G.sumA, gsum_out=self.grad_u, bump_step=-1, **lag)
        elif world is None:
            KN.adam(self.theta.data, G.slabA, st['m'], st['v'], st['step'], lr, gslabB=G.slabB, scal=self.scal,
                    gextraA=acc, gsum_out=self.grad_u, bump_step=-1, **lag)
        else:
            P = self.Pu
            if acc is not None:
                self.pack_u[:P].add_(acc)
            KN.adam(self.theta.data, None, st['m'], st['v'], st['step'], lr, gextraA=self.pack_u[:P],
                    gextraB=self.pack_u[P:2 * P], scal=self.scal, gsum_out=self.grad_u, bump_step=-1, **lag)
        if acc is not None:
            acc.copy_(self.grad_u)

    def xproj_plan(self):
        """how the test network's input layer treats the spatial columns on path-mode groups (solver.plan())"""
        if self.xproj_min_d >= (1 << 30):
            return 'per point (the %s test-network family has no x-projection table)' % ('tiled' if self.testnet_tiled else 'generic')
        if self.d < self.xproj_table_min_d:
            return 'per point (d = %d: the x-projection table is used from d = %d on)' % (self.d, self.xproj_table_min_d)
        if self.xproj_cached:
            return ('x-projection table per path, cached (from d = %d on): formed where the sample is loaded and behind the '
                    'discriminator\'s update, at the head of a launch only when phi or the sample changed otherwise' % self.xproj_table_min_d)
        return 'x-projection table per path, formed at the head of every test-network launch (from d = %d on)' % self.xproj_table_min_d

    def _xproj_held(self, G):
        """does the engine keep G's x-projection table current across sub-steps?  (path mode, caching on)"""
        return self.xproj_cached and G.N > 0 and G.tpp is None and 'xproj' in G._lazy

    def _form_xproj(self, G):
        """G's table from the current phi and sample, on the current stream, and the key it then stands for (called where the
        sample is loaded; the key is host-side bookkeeping like _v_fresh's)"""
        if self._xproj_held(G):
            KN.disc_xproj(G.xvT, self.phi.data, self.W, out=G.xproj)
            G.xproj_key = self._v_key(G)

    def _xproj_tail(self, G):
        """is G's table formed again right behind the discriminator's Adam?  Static per group, but for the carried gradient of a
        sub-iteration over several groups: there phi moves again before G's next sub-step and the launch would be for nothing"""
        return self._xproj_held(G) and self.accum_v is None

    def _xproj_state(self, G, now):
        """python-side bookkeeping (outside the captured graphs): is G's table that of the current phi and sample (`now` = _v_key)?
        Sets G.xproj_cur for the test-network launch of this sub-step -- current: no head launch -- and returns the graph-key suffix"""
        G.xproj_cur = False
        if G.skip_v or not self._xproj_held(G):
            return ''
        G.xproj_cur = getattr(G, 'xproj_key', None) == now
        G.xproj_key = now                # (not current: this sub-step forms it at the head)
        return '_xc' if G.xproj_cur else ''

    def _v_fresh(self, G, store=False):
        """python-side bookkeeping (outside the captured graphs): are the test-network outputs of this group still those
        of the current phi and sample?  Sets G.skip_v for the front segment and returns the graph-key suffix."""
        now = self._v_key(G)
        G.skip_v = self.reuse_test_net and getattr(G, 'v_version', None) == now
        G.v_version = now
        if not G.skip_v:                 # this sub-step evaluates the test network: does it leave the layer inputs behind?
            G.vact_valid = G.vact is not None and (store or self.reuse_test_net)
        return ('_vcached' if G.skip_v else '') + ('_act' if getattr(G, 'vact_valid', False) else '') + self._xproj_state(G, now)

    def _v_key(self, G):
        """(engine-side updates of phi, torch-side in-place writes to its parameters, resamples of the group)"""
        return (self._phi_version, sum(p._version for p in self.phi.params), G.sample_version)

    def invalidate_test_net(self):
        """phi was changed from outside the engine (optimizer_v.step(), load_state_dict, ...)"""
        self._phi_version += 1

    def _run_runner(self, fn, *args):
        from ._lib import check
        self._exchange_error = None
        rc = fn(*args)
        if getattr(self, '_exchange_error', None) is not None:      # (raised inside the host-side exchange stand-in)
            err, self._exchange_error = self._exchange_error, None
            raise err
        check(rc, fn.__name__)

    def generator_step(self, G):
        """one pass of the generator sub-step body; loss_u is left in scal[4] (device)"""
        try:
            self._generator_step(G)
        except BaseException:
            G.xproj_key = None           # (what the bookkeeping promised may not have been launched)
            raise
        finally:
            G.xproj_cur = False          # (a test-network launch outside a sub-step forms its table at the head)

    def _generator_step(self, G):
        sfx = self._v_fresh(G)
        world = self._world_of(G)
        if self._runner_ok(G):
            from ._lib import lib
            skip = self.adam_skips_untouched and not self._field_seen(G)
            G.ck = self.structure.c_kappa
            self._run_runner(lib.xw_substep_gen, self._runner_group(G), self._runner_state(), int(bool(G.skip_v)),
                             int(bool(getattr(G, 'vact_valid', False))), KN._p(self.accum_u), int(skip), KN._stream())
            return
        if world is None:
            self._run(G, 'gen' + sfx, self._gen_all)
            return
        if self.capture_exchange:
            self._run(G, 'gen_dist' + sfx, self._gen_all_dist)
            return
        self._run(G, 'gen_front' + sfx, self._gen_front_packed)   # ... -> pack_u = [sum A | sum B | scal]
        world.all_reduce(self.pack_u)                             # the ONE exchange of the generator sub-step
        self._run(G, 'gen_back', self._gen_back)

    def _gen_all_dist(self, G):
        """several GPUs, capturable exchange: front segment, the ONE all-reduce and the update as one graph"""
        self._gen_front_packed(G)
        self.world.all_reduce(self.pack_u)
        self._gen_back(G)

    def _gen_front_packed(self, G):
        """several GPUs: the front segment ends with the slab sums into the exchange buffer (same captured graph)"""
        P = self.Pu
        if G.N == 0:
            return self._gen_front_empty(G)
        self._gen_front(G)
        KN.slab_sum2(G.slabA, self.pack_u[:P], G.slabB, self.pack_u[P:2 * P])

    def _gen_front_empty(self, G):
        """_gen_front_packed on a rank whose share of the group holds no interior path (fewer paths than ranks): nothing of the
        weak form lives here -- zeros go into the exchange -- but the boundary paths the rank holds, if any, take their forward
        pass and their sweep as usual (csrc/xw_substep.hip does the same for the runner's groups)"""
        P, th = self.Pu, self.theta.data
        M = (self.method, self.H, self.K, self.m)
        self.pack_u.zero_()
        if not G.Nb:
            return
        fwd_b = [self._job(G, 'b')]
        self._ode_fwd_multi(fwd_b, G.tb, th, *M, narrow=self._narrow_ok(fwd_b, alone=False, forward=True))
        sweep_b = [dict(self._job(G, 'b', None, G.slabA[G.ns_u:]), res=self._res_bdry(G))]
        self._ode_bwd_multi(sweep_b, G.tb, th, *M, want_x=False, want_params=True, adjoint=self.adjoint,
                         narrow=self._narrow_ok(sweep_b, alone=False))
        KN.bdry_partials(G.ub, G.g, self.alpha, G.Nbglob, self.scal, G.work_b)
        KN.slab_sum(G.slabA[G.ns_u:], out=self.pack_u[:P])

    # ------------------------------------------------------------------------------------------------------------
    # discriminator sub-step (src/training.py:152-162)
    # ------------------------------------------------------------------------------------------------------------
    def _disc_front(self, G):
        """main: test network (+ its record) -> [join] -> I, sum v^2, loss values;  side 1: u-forward -> x-sweep"""
        th = self.theta.data
        M = (self.method, self.H, self.K, self.m)
        if G.N == 0:                     # an empty share of a sharded group: zeros into both exchanges
            self.scal.zero_()
            return
        e0 = self._mark()
        if not getattr(G, 'skip_v', False):
            self._launch_test_net_here(G, blocks=self.v_blocks_disc)
        with self._side(1, e0):
            # (the only sweep of this sub-step has no weight gradients: the forward stores a seventh of the record)
            fwd = [self._job(G, 'i')]
            lone = bool(getattr(G, 'skip_v', False))          # (the test network is reused: this chain has the chip to itself)
            self._ode_fwd_multi(fwd, G.t, th, *M, zero16=self.scal, act_x_only=True, narrow=self._narrow_ok(fwd, alone=lone, forward=True),
                             prio_drop=self.prio_drop['F'])
            self._reaction(G)
            sweep_x = [self._job(G, 'i', want_x=True)]
            self._ode_bwd_multi(sweep_x, G.t, th, *M, want_x=True, want_params=False, adjoint=self.adjoint,
                             narrow=self._narrow_ok(sweep_x, alone=lone, params=False), prio_drop=self.prio_drop['X'])
            e_x = self._mark()
        self._join(e_x)
        self._contract(G, self.adam_v)

    def _disc_mid(self, G):
        KN.disc_cotangent(G.u, G.v, G.w, G.f, G.h, G.Vol, G.Nglob, self.scal, G.vbar, c=G.c, ckappa=G.ck,
                          pollution=self.pollution, s3_scale=G.s3_scale)
        act = G.vact if getattr(G, 'vact_valid', False) else None
        if G.tpp is None:
            KN.disc_bwd(G.xvT, G.t, self.phi.data, G.vbar, self.W, self.q, gslab=G.slab_v, act=act)
        else:
            KN.disc_bwd(G.xvT_pts, None, self.phi.data, G.vbar.view(1, -1), self.W, self.q, tpp=G.tpp, gslab=G.slab_v, act=act)

    def _disc_mid_packed(self, G):
        if G.N == 0:
            self.grad_v.zero_()
            return
        self._disc_mid(G)
        KN.slab_sum(G.slab_v, out=self.grad_v)

    def _disc_back(self, G):
        lr, st = self.config['v_rate'], self.adam_v
        acc = self.accum_v
        world = self._world_of(G)
        if world is not None:
            KN.losses(self.scal, G.L, G.Lb, G.Vol, G.Nglob, G.Nbglob, self.alpha, step=st['step'])
        if world is None:
            KN.adam(self.phi.data, G.slab_v, st['m'], st['v'], st['step'], lr, gextraA=acc, gsum_out=self.grad_v,
                    bump_step=-1)
        else:
            if acc is not None:
                self.grad_v.add_(acc)
            KN.adam(self.phi.data, None, st['m'], st['v'], st['step'], lr, gextraA=self.grad_v, bump_step=-1)
        if self._xproj_tail(G):
            # phi has just moved: G's table for the sub-steps that follow, on the same queue directly behind the update (a same-queue
            # successor starts without a gap; at the head of the next sub-step it would be one more dependent node of its critical chain)
            KN.disc_xproj(G.xvT, self.phi.data, self.W, out=G.xproj)
        if acc is not None:
            acc.copy_(self.grad_v)

    def _reduce_sums(self, G):
        """several GPUs: the partial sums I, sum v^2, SSE (+ the two factors of a pairwise group's d(phi)/dt term, folded
        into I once they are global)"""
        self.world.all_reduce(self.scal[0:9])
        if G.pair_i:
            KN.pair_fold(self.scal, G.Vol, G.Nglob)

    def _disc_all(self, G):
        self._disc_front(G)
        self._disc_mid(G)
        self._disc_back(G)

    def _disc_all_dist(self, G):
        """several GPUs, capturable exchanges: the whole discriminator sub-step with its two all-reduces as one graph"""
        self._disc_front(G)
        self._reduce_sums(G)
        self._disc_mid_packed(G)
        self.world.all_reduce(self.grad_v)
        self._disc_back(G)

    def discriminator_step(self, G):
        """one pass of the discriminator sub-step body; loss_v is left in scal[5] (device)"""
        try:
            self._discriminator_step(G)
        except BaseException:
            G.xproj_key = None
            raise
        finally:
            G.xproj_cur = False

    def _disc_bookkeeping(self, G):
        """host side of a discriminator sub-step, outside captured code: the graph-key suffix, phi's version, the table's key"""
        sfx = self._v_fresh(G, store=True)
        self._phi_version += 1                                    # phi changes at the end of this sub-step
        if self._xproj_tail(G):
            G.xproj_key = self._v_key(G)                          # ... and G's table is formed again right behind that update
        return sfx

    def _discriminator_step(self, G):
        sfx = self._disc_bookkeeping(G)
        world = self._world_of(G)
        if self._runner_ok(G):
            from ._lib import lib
            G.ck = self.structure.c_kappa
            self._run_runner(lib.xw_substep_disc, self._runner_group(G), self._runner_state(), int(bool(G.skip_v)),
                             int(bool(getattr(G, 'vact_valid', False))), KN._p(self.accum_v), KN._stream())
            return
        if world is None:
            self._run(G, 'disc' + sfx, self._disc_all)
            return
        if self.capture_exchange:
            self._run(G, 'disc_dist' + sfx, self._disc_all_dist)
            return
        self._run(G, 'disc_front' + sfx, self._disc_front)
        self._reduce_sums(G)                                      # I and sum v^2 must be global before the cotangent
        self._run(G, 'disc_mid' + ('_act' if getattr(G, 'vact_valid', False) else ''), self._disc_mid_packed)
        world.all_reduce(self.grad_v)
        self._run(G, 'disc_back', self._disc_back)

    # ------------------------------------------------------------------------------------------------------------
    def _run(self, G, key, fn, scratch=False):
        """execute fn(G) eagerly, or capture it once into a HIP graph (per group and segment) and replay it.
        scratch: fn allocates while it runs and leaves nothing behind in what it allocated (True / 1: scratch pool 0, 2: pool 1)"""
        # (a pairwise group carries per-sample host constants -- the variance offsets -- into its launches: never captured)
        capturable = (self.use_graphs and self.accum_u is None and self.accum_v is None and getattr(G, 'persistent', True)
                      and not (G.pair_i or G.pair_b))
        g = G.graphs.get(key) if capturable else False
        if g is False:                            # not capturable, or capture of THIS segment was refused before
            if not getattr(G, 'persistent', True) and self.use_streams:
                # a group of a list domain (new shapes every sample: eager launches, issued faster than the small kernels
                # run out): one stream -- the side-stream contexts and events cost more host time than the overlap returns
                # (cone outer iteration 28.5 -> 25.4 ms, hourglass 57.5 -> 52.4 ms)
                self.use_streams = False
                # (operand validation: every launch of the first `eager_checked` eager segments -- a few outer iterations --
                #  then the engine trusts its own buffers, kernels.TRUSTED; XW_ALWAYS_CHECK=1 keeps validating)
                self._eager_seen = getattr(self, '_eager_seen', 0) + 1
                KN.TRUSTED = self._eager_seen > self.eager_checked
                try:
                    fn(G)
                finally:
                    self.use_streams = True
                    KN.TRUSTED = False
                return
            fn(G)
            return
        if g is None:
            ran_eager = self.structure.c_kappa is None
            if ran_eager:
                fn(G)                             # a black-box c(u, t, x): one eager pass first (allocations, lazy init of its ops)
            g = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            try:
                # thread_local: other threads (the RCCL watchdog polls events) must not invalidate the capture
                # (HIP_HOST_LOCK: no page-locked allocation of the sampling helper thread during a capture or a launch)
                with HIP_HOST_LOCK, torch.cuda.graph(g, pool=_scratch_pool(int(scratch) - 1) if scratch else None, stream=self._capture_stream(),
                                                     capture_error_mode='thread_local'):
                    fn(G)
            except Exception as exc:
                # Capture refused (typically a user callable that syncs with the host or builds CPU tensors): THIS segment
                # of THIS group runs eagerly from now on -- several times slower, so say it loudly, once per segment, and
                # leave every other segment captured (XW_STRICT_GRAPHS=1 turns the cliff into an error)
                if self.options.strict_graphs:
                    raise
                import warnings
                warnings.warn('HIP graph capture of sub-step segment %r failed (%s: %s); this segment now runs as eager kernel launches '
                              '(expect a several times lower step rate)' % (key, type(exc).__name__, exc), RuntimeWarning, stacklevel=2)
                G.graphs[key] = False
                self.eager_segments = getattr(self, 'eager_segments', 0) + 1
                torch.cuda.synchronize()
                if not ran_eager:                 # (with a black-box c the eager pass above already WAS this call's step:
                    fn(G)                         #  running fn again would apply a second optimiser update)
                return
            G.graphs[key] = g
            _KEPT_GRAPHS.append(g)                # (never destroyed: see _KEPT_GRAPHS)
            if len(_KEPT_GRAPHS) in (256, 1024, 4096):
                import warnings
                # a process that builds many solvers (hyper-parameter sweeps) or whose group shapes keep changing: every graph
                # and its private memory pool stay until exit
                warnings.warn('%d captured HIP graphs are being kept alive (destroying one faults a later launch on this runtime, '
                              'engine._KEPT_GRAPHS): a long-lived process that keeps building solvers should run them with '
                              'XW_GRAPHS=0 or in child processes' % len(_KEPT_GRAPHS), RuntimeWarning, stacklevel=3)
            if ran_eager:
                return                            # (the eager pass above was this call's step; the capture only recorded)
        with HIP_HOST_LOCK:
            g.replay()

    def _capture_stream(self):
        return self._cap

    def loss_u(self):
        return self.scal[4]

    def loss_v(self):
        return self.scal[5]

    # ---- the stepper launches, for every served solver ------------------------------------------------------------
    def _ode_fwd_multi(self, jobs, t, th, method, H, K, m, zero16=None, **kw):
        """KN.ode_fwd_multi; with dopri5 one kernels.dopri5_fwd per 8 jobs, each job's step record kept for its sweep
        (keyed by the job's sample and grid, which the sweep jobs share)"""
        if self.tiled and method != KN.DOPRI5:
            return KN.tiled_ode_fwd_multi(jobs, t, th, method, H, K, m, zero16=zero16, **kw)
        if method != KN.DOPRI5:
            return KN.ode_fwd_multi(jobs, t, th, method, H, K, m, zero16=zero16, **kw)
        if zero16 is not None:
            zero16.zero_()
        o = self.options
        for i in range(0, len(jobs), KN.DOPRI5_MAXJOBS):
            part = jobs[i:i + KN.DOPRI5_MAXJOBS]
            recs = KN.dopri5_fwd([dict(xT=j['xT'], start=j['start'], u=j['u'], Y=j.get('Y')) for j in part], t, th, H, K, m,
                                 self.config['u_hidden_dim'], chunk=o.dopri5_chunk, max_steps=o.dopri5_max_steps,
                                 stepper=self.dopri5_stepper)
            for j, r in zip(part, recs):
                self._dopri_recs[(j['xT'].data_ptr(), t.data_ptr())] = r

    def _ode_bwd_multi(self, jobs, t, th, method, H, K, m, want_x, want_params, x_cot_ones=False, adjoint=False, **kw):
        """KN.ode_bwd_multi; with dopri5 kernels.dopri5_sweep over the records of the forward that produced these jobs' u"""
        if self.tiled and method != KN.DOPRI5:
            return KN.tiled_ode_bwd_multi(jobs, t, th, method, H, K, m, want_x, want_params, x_cot_ones=x_cot_ones, adjoint=adjoint, **kw)
        if method != KN.DOPRI5:
            return KN.ode_bwd_multi(jobs, t, th, method, H, K, m, want_x, want_params, x_cot_ones=x_cot_ones, adjoint=adjoint, **kw)
        for i in range(0, len(jobs), KN.DOPRI5_MAXJOBS):
            part = [dict(j, rec=self._dopri_recs[(j['xT'].data_ptr(), t.data_ptr())]) for j in jobs[i:i + KN.DOPRI5_MAXJOBS]]
            KN.dopri5_sweep(part, t, th, H, K, m, want_x, want_params, x_cot_ones=x_cot_ones, stepper=self.dopri5_stepper)

    def _u_forward(self, xT, t, start):
        return KN.u_forward(xT, t, start, self.theta.data, self.method, self.H, self.K, self.m, self.config['u_hidden_dim'], family=self.stepper,
                            chunk=self.options.dopri5_chunk, max_steps=self.options.dopri5_max_steps, stepper=self.dopri5_stepper)

    def predict_group(self, G):
        """u_theta on the interior paths of a loaded group as the module returns it, [N, L, 1] -- no path tensor, no callables:
        the group already holds the transposed points, the grid and the start values"""
        return self._u_forward(G.xT, G.t, G.start).t().unsqueeze(2)

    def predict(self, X):
        """u_theta on a group [N, L, d+1] -> [L, N] (diagnostics; no checkpoints kept)"""
        Xd = X.detach()
        s = start_values(self.funcs, Xd[:, 0, :], at_T0(self.setup['T0'], first=Xd[0, 0, 0]), False)
        return self._u_forward(Xd[:, 0, 1:].to(self.dev).to(F64).t().contiguous(), Xd[0, :, 0].to(self.dev).to(F64).contiguous(),
                               s.detach().to(self.dev).to(F64).reshape(-1).contiguous())

    def predict_paths(self, X, starts=None):
        """u_theta on a RAGGED group [N, L, 1 + d] -> [L, N]: every path integrates over its OWN time channel X[i, :, 0]
        (non-decreasing; a shorter path repeats its last time, and its padded rows hold its final value), x from slice 0 as the
        module reads it.  starts [N]: the start values; None: per path h where X[i, 0, 0] == T0, else g -- the batched form of
        evaluating [[x0, x]] point by point.  On the tiled family's per-path kernel (kernels.tiled_paths_fwd) at the blob's
        widths, whichever family trains; fixed-grid schemes only; EngineOptions.eval_chunk_paths paths per launch."""
        from . import evalpaths
        if self.method not in KN.METHODS.values():
            raise XnwanError("predict_paths: solver %r is not served -- per-path time grids run the fixed-grid schemes %s only%s"
                             % (self.config['solver'], sorted(KN.METHODS),
                                " (dopri5's per-path step controller, kernels.paths_dopri5_fwd, gives one output time per path: "
                                "solver.evaluate; several output times per path are not built)" if self.method == KN.DOPRI5 else ''))
        with torch.no_grad():
            Xd = X.detach()
            if Xd.dim() != 3 or Xd.shape[2] != 1 + self.d:
                raise XnwanError('predict_paths: X must be [N, L, 1 + d] = [N, L, %d]' % (1 + self.d))
            tT = Xd[:, :, 0].to(self.dev).to(F64).t().contiguous()
            if starts is None:
                first = Xd[:, 0, :]
                at_T0 = first[:, 0] == self.setup['T0']
                if bool(at_T0.all()):
                    starts = self.funcs['h'](first)
                else:
                    starts = torch.where(at_T0, self.funcs['h'](first).reshape(-1), self.funcs['g'](first.unsqueeze(1)).reshape(-1))
            if tT.shape[0] > 1 and bool((tT[1:] < tT[:-1]).any()):      # (the one device-side check)
                raise XnwanError('predict_paths: the times of a path must not decrease')
            return evalpaths.paths_forward(Xd[:, 0, 1:].to(self.dev).to(F64).t().contiguous(), tT,
                                           starts.detach().to(self.dev).to(F64).reshape(-1).contiguous(), evalpaths.last_distinct(tT),
                                           self.theta.data, self.method, self.H, self.K, self.m,
                                           chunk=self.options.eval_chunk_paths)
