"""ctypes binding of libxnwan.so (C ABI declared in include/xnwan.h).

The library is the product: there is no CPU or eager-PyTorch fallback.  Importing this module without the built
library raises, and so does any call when no GPU is present.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('XW_LIBRARY') or os.path.join(_HERE, 'libxnwan.so')   # (override: kernel experiments only)
ABI_VERSION = 33

c_f32p = ctypes.c_void_p   # coordinates / time grid: const double* (device)   [name kept from the float32 era]
c_f64p = ctypes.c_void_p   # double*       (device)
c_i64p = ctypes.c_void_p
c_int, c_dbl, c_vp = ctypes.c_int, ctypes.c_double, ctypes.c_void_p


class XwOdeFwdJob(ctypes.Structure):      # include/xnwan.h
    _fields_ = [('xT', c_vp), ('start', c_vp), ('u', c_vp), ('Y', c_vp), ('act', c_vp), ('N', c_int), ('act_x_only', c_int),
                ('narrow', c_int), ('prio_drop', c_int)]


class XwOdeBwdJob(ctypes.Structure):
    _fields_ = [('xT', c_vp), ('start', c_vp), ('Y', c_vp), ('act', c_vp), ('ubar', c_vp), ('gx', c_vp), ('gs', c_vp),
                ('gslab', c_vp), ('N', c_int), ('res_first_only', c_int), ('res_u', c_vp), ('res_ref', c_vp),
                ('res_coef', ctypes.c_double), ('res_base', ctypes.c_double), ('res_w_per_point', c_int), ('res_w', c_vp),
                ('res_c', c_vp), ('res_cp', c_vp), ('res_kappa2', ctypes.c_double), ('res_scal', c_vp), ('res_refA', c_vp),
                ('res_coefA', ctypes.c_double), ('res_baseA', ctypes.c_double)]


class XwPathsJob(ctypes.Structure):       # include/xnwan.h: one ragged group of xw_paths_tiled_fwd (a time grid per path)
    _fields_ = [('xT', c_vp), ('start', c_vp), ('tT', c_vp), ('nstep', c_vp), ('u', c_vp), ('Y', c_vp), ('N', c_int),
                ('last_only', c_int)]


class XwPathsDopriJob(ctypes.Structure):  # include/xnwan_eval.h: one group of xw_paths_dopri5_fwd (a step controller per path)
    _fields_ = [('xT', c_vp), ('start', c_vp), ('t_in', c_vp), ('t_end', c_vp), ('u', c_vp), ('status', c_vp), ('n_acc', c_vp),
                ('n_att', c_vp), ('Y', c_vp), ('rec', c_vp), ('fin', c_vp), ('N', c_int), ('cap', c_int)]


class XwPathsGradJob(ctypes.Structure):   # include/xnwan_grad.h: one ragged group of xw_paths_tiled_grad (the sweep behind XwPathsJob)
    _fields_ = [('xT', c_vp), ('start', c_vp), ('tT', c_vp), ('nstep', c_vp), ('Y', c_vp), ('gx', c_vp), ('gs', c_vp), ('ut', c_vp),
                ('N', c_int)]


class XwPathsHvpJob(ctypes.Structure):    # include/xnwan_hess.h: one ragged group of xw_paths_tiled_hvp (XwPathsGradJob's inputs and a direction)
    _fields_ = [('xT', c_vp), ('start', c_vp), ('tT', c_vp), ('nstep', c_vp), ('Y', c_vp), ('vx', c_vp), ('vs', c_vp), ('Yd', c_vp),
                ('ju', c_vp), ('hx', c_vp), ('hs', c_vp), ('N', c_int)]


class XwPathsJetJob(ctypes.Structure):    # include/xnwan_jet.h: one ragged group of xw_paths_tiled_jet (XwPathsJob's inputs, R curves per path, no Y)
    _fields_ = [('xT', c_vp), ('start', c_vp), ('tT', c_vp), ('nstep', c_vp), ('vx', c_vp), ('vs', c_vp), ('qs', c_vp), ('u', c_vp),
                ('ju', c_vp), ('quu', c_vp), ('N', c_int), ('R', c_int)]


class XwPathsVjpJob(ctypes.Structure):    # include/xnwan_vjp.h: one ragged group of xw_paths_tiled_vjp (XwPathsGradJob's inputs, a weight per path, slabs)
    _fields_ = [('xT', c_vp), ('start', c_vp), ('tT', c_vp), ('nstep', c_vp), ('Y', c_vp), ('w', c_vp), ('gslab', c_vp), ('gx', c_vp),
                ('gs', c_vp), ('N', c_int)]


class XwPathsGvjpJob(ctypes.Structure):   # include/xnwan_grad_vjp.h: one ragged group of xw_paths_tiled_gvjp (XwPathsHvpJob's inputs with Yd read, two weights per path, slabs)
    _fields_ = [('xT', c_vp), ('start', c_vp), ('tT', c_vp), ('nstep', c_vp), ('Y', c_vp), ('Yd', c_vp), ('vx', c_vp), ('vs', c_vp),
                ('wu', c_vp), ('wt', c_vp), ('gslab', c_vp), ('N', c_int)]


class XwPathsDopriCkptJob(ctypes.Structure):  # include/xnwan_eval_grad.h: XwPathsDopriJob with the checkpoints kept (f.cap slots)
    _fields_ = [('f', XwPathsDopriJob), ('ckpt', c_vp)]


class XwPathsDopriGradJob(ctypes.Structure):   # include/xnwan_eval_grad.h: one group of xw_paths_dopri5_grad (the sweep behind it)
    _fields_ = [('xT', c_vp), ('start', c_vp), ('t_in', c_vp), ('t_end', c_vp), ('n_acc', c_vp), ('rec', c_vp), ('ckpt', c_vp),
                ('Y', c_vp), ('gx', c_vp), ('gs', c_vp), ('ut', c_vp), ('N', c_int), ('cap', c_int)]


class XwDopriJob(ctypes.Structure):       # include/xnwan.h: solver 'dopri5', one job of the forward launches
    _fields_ = [('xT', c_vp), ('start', c_vp), ('u', c_vp), ('Y', c_vp), ('rec_y', c_vp), ('rec_t', c_vp), ('rec_h', c_vp),
                ('fbuf', c_vp), ('ctl', c_vp), ('work', c_vp), ('N', c_int), ('cap', c_int)]


class XwDopriSweepJob(ctypes.Structure):  # ... and of the sweep
    _fields_ = [('b', XwOdeBwdJob), ('rec_y', c_vp), ('rec_t', c_vp), ('rec_h', c_vp), ('ctl', c_vp)]


class XwGroup(ctypes.Structure):           # include/xnwan.h: one group of paths for xw_substep_gen / xw_substep_disc
    _fields_ = ([(n, c_int) for n in ('N', 'Nb', 'L', 'Lb', 'd', 'same_grid', 'w_per_point', 'amode', 'pair_i', 'pair_b', 'ns_u', 'ns_b',
                                      'narrow', 'sharded')]
                + [(n, c_dbl) for n in ('Vol', 'Nglob', 'Nbglob', 's3_scale', 'init_off', 'bdry_off', 'ckappa')]
                + [(n, c_vp) for n in ('xT', 'xvT', 'xbT', 't', 'tb', 'tpp', 'xvT_pts', 'start', 'start_b', 'h', 'href', 'f', 'g', 'w',
                                       'wt', 'w0', 'ghT', 'gwx0T', 'c', 'cp', 'A0', 'B0', 'u', 'ub', 'Y', 'Yb', 'act', 'act_b', 'v',
                                       'vt', 'gxv', 'gtv', 'gx', 'gs', 'vbar', 's3x', 'vact', 'slabA', 'slabB', 'slab_v', 'work_i',
                                       'work_b', 'xproj')]
                + [('xproj_current', c_int)])


class XwSolverState(ctypes.Structure):
    _fields_ = ([(n, c_int) for n in ('method', 'H', 'K', 'm', 'W', 'q', 'Pu', 'Pv', 'adjoint', 'v_blocks', 'v_blocks_disc', 'lag_lo',
                                      'lag_hi')]
                + [(n, c_dbl) for n in ('alpha', 'pollution', 'lr_u', 'lr_v', 'beta1', 'beta2', 'eps')]
                + [(n, c_vp) for n in ('theta', 'phi', 'scal', 'grad_u', 'grad_v', 'm_u', 'v_u', 'm_v', 'v_v', 'step_u', 'step_v',
                                       'lag_u', 'exchange', 'exchange_ctx', 'pack_u')]
                + [('merged_sweep', c_int)])


# XwSolverState.exchange: int (*)(double* buf, int count, void* ctx, void* stream) -- xw_allreduce's own signature
EXCHANGE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p)


# name -> argument types (return type is always int); mirrors include/xnwan.h line by line
SIGNATURES = {
    'xw_abi_version': [],
    'xw_supported_dims': [ctypes.c_char_p, c_int],
    'xw_theta_size': [c_int, c_int, c_int],
    'xw_phi_size': [c_int, c_int],
    'xw_ode_fwd': [c_f32p, c_f32p, c_f64p, c_f64p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_f64p, c_f64p, c_vp],
    'xw_ode_fwd_multi': [ctypes.POINTER(XwOdeFwdJob), c_int, c_f32p, c_f64p, c_int, c_int, c_int, c_int, c_int, c_int, c_f64p,
                         c_vp],
    'xw_ode_bwd_slabs': [c_int],
    'xw_ode_act_rows': [c_int, c_int, c_int, c_int],
    'xw_ode_bwd_multi': [ctypes.POINTER(XwOdeBwdJob), c_int, c_f32p, c_f64p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_vp],
    'xw_tiled_ode_ok': [c_int, c_int, c_int, c_int],
    'xw_tiled_ode_work': [c_int, c_int, c_int, c_int, c_int],
    'xw_tiled_ode_bwd_slabs': [c_int],
    'xw_tiled_ode_fwd_multi': [ctypes.POINTER(XwOdeFwdJob), c_int, c_f32p, c_f64p, c_int, c_int, c_int, c_int, c_int, c_int, c_f64p,
                               c_f64p, c_vp],
    'xw_tiled_ode_bwd_multi': [ctypes.POINTER(XwOdeBwdJob), c_int, c_f32p, c_f64p, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                               c_f64p, c_vp],
    'xw_paths_tiled_work': [c_int, c_int, c_int, c_int],
    'xw_paths_tiled_fwd': [ctypes.POINTER(XwPathsJob), c_int, c_f64p, c_int, c_int, c_int, c_int, c_int, c_int, c_f64p, c_vp],
    'xw_adams_coef': [c_int, c_vp],
    'xw_adams_tiled_work': [c_int, c_int, c_int, c_int, c_int],
    'xw_adams_tiled_fwd_multi': [ctypes.POINTER(XwOdeFwdJob), c_int, c_f32p, c_f64p, c_int, c_int, c_int, c_int, c_int, c_f64p, c_f64p,
                                 c_vp],
    'xw_adams_tiled_bwd_multi': [ctypes.POINTER(XwOdeBwdJob), c_int, c_f32p, c_f64p, c_int, c_int, c_int, c_int, c_int, c_int, c_f64p,
                                 c_vp],
    'xw_dopri5_ctl_size': [],
    'xw_dopri5_work_size': [c_int],
    'xw_dopri5_init': [ctypes.POINTER(XwDopriJob), c_int, c_f32p, c_f64p, c_int, c_int, c_int, c_int, c_int, c_int, c_dbl, c_dbl,
                       c_vp],
    'xw_dopri5_attempts': [ctypes.POINTER(XwDopriJob), c_int, c_f32p, c_f64p, c_int, c_int, c_int, c_int, c_int, c_int, c_dbl,
                           c_dbl, c_int, c_int, c_vp],
    'xw_dopri5_sweep': [ctypes.POINTER(XwDopriSweepJob), c_int, c_f32p, c_f64p, c_int, c_int, c_int, c_int, c_int, c_int, c_vp],
    'xw_tdopri5_work': [c_int, c_int, c_int, c_int, c_int],
    'xw_tdopri5_part_size': [c_int],
    'xw_tdopri5_init': [ctypes.POINTER(XwDopriJob), c_int, c_f32p, c_f64p, c_int, c_int, c_int, c_int, c_int, c_int, c_dbl, c_dbl,
                        c_f64p, c_vp],
    'xw_tdopri5_attempts': [ctypes.POINTER(XwDopriJob), c_int, c_f32p, c_f64p, c_int, c_int, c_int, c_int, c_int, c_int, c_dbl,
                            c_dbl, c_int, c_int, c_f64p, c_vp],
    'xw_tdopri5_sweep': [ctypes.POINTER(XwDopriSweepJob), c_int, c_f32p, c_f64p, c_int, c_int, c_int, c_int, c_int, c_int, c_f64p,
                         c_vp],
    'xw_ode_bwd': [c_f32p, c_f32p, c_f64p, c_f64p, c_f64p, c_f64p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                   c_f64p, c_f64p, c_f64p, c_vp],
    'xw_disc_fwd': [c_f32p, c_f32p, c_f32p, c_f64p, c_int, c_int, c_int, c_int, c_int, c_f64p, c_f64p, c_f64p, c_f64p, c_int,
                    c_int, c_f64p, c_vp],
    'xw_disc_xproj': [c_f32p, c_f64p, c_int, c_int, c_int, c_f64p, c_vp],
    'xw_disc_fwd_xproj': [c_f32p, c_f32p, c_f32p, c_f64p, c_int, c_int, c_int, c_int, c_int, c_f64p, c_f64p, c_f64p, c_f64p, c_int,
                          c_int, c_f64p, c_f64p, c_vp],
    'xw_disc_act_rows': [c_int, c_int],
    'xw_disc_gradx': [c_f32p, c_f32p, c_f32p, c_f64p, c_f64p, c_int, c_int, c_int, c_int, c_f64p, c_f64p, c_vp],
    'xw_disc_bwd_slabs': [c_int, c_int],
    'xw_disc_bwd': [c_f32p, c_f32p, c_f32p, c_f64p, c_f64p, c_int, c_int, c_int, c_int, c_int, c_f64p, c_f64p, c_vp],
    'xw_disc_tiled_ok': [c_int, c_int, c_int],
    'xw_disc_tiled_act_rows': [c_int, c_int],
    'xw_disc_tiled_fwd': [c_f32p, c_f32p, c_f32p, c_f64p, c_int, c_int, c_int, c_int, c_int, c_f64p, c_f64p, c_f64p, c_f64p, c_int,
                          c_int, c_f64p, c_f64p, c_vp],
    'xw_disc_tiled_bwd': [c_f32p, c_f32p, c_f32p, c_f64p, c_f64p, c_int, c_int, c_int, c_int, c_int, c_f64p, c_f64p, c_vp],
    'xw_mt19937_uniform_f32': [c_vp, ctypes.c_long, c_vp, ctypes.c_long, ctypes.c_float, ctypes.c_float, c_int],
    'xw_gather_fields': [c_vp, c_int, ctypes.c_long, c_vp],
    'xw_mt19937_legacy_normal_f64': [c_vp, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_dbl), c_vp, ctypes.c_long],
    'xw_weak_partials': [c_f64p, c_f64p, c_f64p, c_f64p, c_int, c_f64p, c_f64p, c_f64p, c_f64p, c_f64p, c_f64p, c_f64p,
                         c_f64p, c_int, c_f64p, c_dbl, c_f64p, c_f64p, c_f64p, c_int, c_dbl, c_int, c_int, c_dbl, c_dbl, c_f64p, c_f64p,
                         c_int, c_int, c_dbl, c_dbl, c_dbl, c_dbl, c_i64p, c_f64p, c_f64p, ctypes.c_long, c_vp],
    'xw_pair_fold': [c_f64p, c_dbl, c_dbl, c_vp],
    'xw_cube_weight': [c_vp, c_int, c_int, c_dbl, c_dbl, c_f64p, c_f64p, c_f64p, c_f64p, c_vp],
    'xw_bdry_partials': [c_f64p, c_f64p, c_int, c_int, c_dbl, c_dbl, c_f64p, c_f64p, c_f64p, c_vp],
    'xw_reduce_work_size': [],
    'xw_weak_contract_general': [c_f64p, c_int, c_f64p, c_f64p, c_f64p, c_f64p, c_f64p, c_f64p, c_f64p, c_f64p, c_int, c_int, c_f64p, c_vp],
    'xw_gen_cotangents': [c_f64p, c_f64p, c_f64p, c_int, c_f64p, c_f64p, c_dbl, c_f64p, c_int, c_int, c_dbl, c_dbl, c_dbl,
                          c_dbl, c_f64p, c_f64p, c_f64p, c_vp],
    'xw_disc_cotangent': [c_f64p, c_f64p, c_f64p, c_int, c_f64p, c_dbl, c_f64p, c_f64p, c_int, c_int, c_dbl, c_dbl, c_dbl,
                          c_dbl, c_f64p, c_f64p, c_vp],
    'xw_losses': [c_f64p, c_int, c_int, c_dbl, c_dbl, c_dbl, c_dbl, c_dbl, c_dbl, c_i64p, c_vp],
    'xw_adam': [c_f64p, c_f64p, c_int, c_f64p, c_f64p, c_int, c_f64p, c_f64p, c_f64p, c_f64p, c_i64p, c_int, c_int, c_dbl,
                c_dbl, c_dbl, c_dbl, c_f64p, c_int, c_int, c_int, c_i64p, c_vp],
    'xw_substep_gen': [ctypes.POINTER(XwGroup), ctypes.POINTER(XwSolverState), c_int, c_int, c_f64p, c_int, c_vp],
    'xw_substep_disc': [ctypes.POINTER(XwGroup), ctypes.POINTER(XwSolverState), c_int, c_int, c_f64p, c_vp],
    'xw_slab_sum': [c_f64p, c_int, c_int, c_int, c_f64p, c_vp],
    'xw_slab_sum2': [c_f64p, c_int, c_f64p, c_f64p, c_int, c_f64p, c_int, c_vp],
    'xw_comm_available': [],
    'xw_comm_unique_id': [ctypes.c_char_p],
    'xw_comm_init': [ctypes.c_char_p, c_int, c_int, ctypes.POINTER(c_vp)],
    'xw_allreduce': [c_f64p, c_int, c_vp, c_vp],
    'xw_comm_destroy': [c_vp],
}

# the extension header include/xnwan_eval.h (include/xnwan.h and SIGNATURES above are frozen at ABI_VERSION): same conventions
EVAL_SIGNATURES = {
    'xw_paths_dopri5_work': [c_int, c_int, c_int, c_int],
    'xw_paths_dopri5_fwd': [ctypes.POINTER(XwPathsDopriJob), c_int, c_f64p, c_int, c_int, c_int, c_int, c_int, c_dbl, c_dbl, c_int,
                            c_int, c_f64p, c_vp],
}

# the extension header include/xnwan_grad.h: same conventions
GRAD_SIGNATURES = {
    'xw_paths_tiled_grad_work': [c_int, c_int, c_int, c_int],
    'xw_paths_tiled_grad': [ctypes.POINTER(XwPathsGradJob), c_int, c_f64p, c_int, c_int, c_int, c_int, c_int, c_int, c_f64p, c_vp],
}


# the extension header include/xnwan_eval_grad.h: same conventions
EVAL_GRAD_SIGNATURES = {
    'xw_paths_dopri5_ckpt_fwd': [ctypes.POINTER(XwPathsDopriCkptJob), c_int, c_f64p, c_int, c_int, c_int, c_int, c_int, c_dbl, c_dbl,
                                 c_int, c_int, c_f64p, c_vp],
    'xw_paths_dopri5_grad_work': [c_int, c_int, c_int, c_int],
    'xw_paths_dopri5_grad': [ctypes.POINTER(XwPathsDopriGradJob), c_int, c_f64p, c_int, c_int, c_int, c_int, c_f64p, c_vp],
}


# the extension header include/xnwan_hess.h: same conventions
HESS_SIGNATURES = {
    'xw_paths_tiled_hvp_work': [c_int, c_int, c_int, c_int],
    'xw_paths_tiled_hvp': [ctypes.POINTER(XwPathsHvpJob), c_int, c_f64p, c_int, c_int, c_int, c_int, c_int, c_int, c_f64p, c_vp],
}


# the extension header include/xnwan_jet.h: same conventions
JET_SIGNATURES = {
    'xw_paths_tiled_jet_work': [c_int, c_int, c_int, c_int],
    'xw_paths_tiled_jet': [ctypes.POINTER(XwPathsJetJob), c_int, c_f64p, c_int, c_int, c_int, c_int, c_int, c_int, c_f64p, c_vp],
}


# the extension header include/xnwan_vjp.h: same conventions
VJP_SIGNATURES = {
    'xw_paths_tiled_vjp_work': [c_int, c_int, c_int, c_int],
    'xw_paths_tiled_vjp': [ctypes.POINTER(XwPathsVjpJob), c_int, c_f64p, c_int, c_int, c_int, c_int, c_int, c_int, c_f64p, c_vp],
}


# the extension header include/xnwan_grad_vjp.h: same conventions
GVJP_SIGNATURES = {
    'xw_paths_tiled_gvjp_work': [c_int, c_int, c_int, c_int],
    'xw_paths_tiled_gvjp': [ctypes.POINTER(XwPathsGvjpJob), c_int, c_f64p, c_int, c_int, c_int, c_int, c_int, c_int, c_f64p, c_vp],
}


class XwSwitches(ctypes.Structure):    # include/xnwan_switches.h: the library's process-wide switches
    _fields_ = [(n, c_int) for n in ('disc_dynamic', 'disc_vin_lds', 'disc_rec_tsum', 'duo_spread', 'reduce_blocks', 'reduce_threads')]


# the extension header include/xnwan_switches.h: same conventions
SWITCH_SIGNATURES = {
    'xw_switches_set': [ctypes.POINTER(XwSwitches)],
    'xw_switches_get': [ctypes.POINTER(XwSwitches)],
}

ERRORS = {-1: 'XW_E_DIMS: network widths/depths not among the compiled kernel instantiations',
          -2: 'XW_E_ARG: null pointer, non-positive size or bad enum',
          -3: 'XW_E_WORKSPACE: workspace too small',
          -4: 'XW_E_COMM: RCCL is not available in this process, or a collective call failed'}


class XnwanError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise XnwanError(
            'libxnwan.so not found at %s -- build it with `python -c "import __graft_entry__ as g; g.build()"` '
            'or `make -C xnode_wan_pde_solver_amd/csrc`.  There is no CPU fallback.' % LIB_PATH)
    # torch FIRST: its wheel ships its own ROCm runtime (torch/lib/libamdhip64.so); loaded before torch, this library would pull in
    # the system's copy and the process would hold two HIP runtimes -- its kernels registered with one, torch's streams and memory
    # living in the other (every launch then fails with hipErrorNoDevice: build() followed by smoke() in ONE process did)
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in (list(SIGNATURES.items()) + list(EVAL_SIGNATURES.items()) + list(GRAD_SIGNATURES.items())
                           + list(EVAL_GRAD_SIGNATURES.items()) + list(HESS_SIGNATURES.items()) + list(JET_SIGNATURES.items())
                           + list(VJP_SIGNATURES.items()) + list(GVJP_SIGNATURES.items()) + list(SWITCH_SIGNATURES.items())):
        fn = getattr(lib, name)           # AttributeError here = the .so does not export the declared ABI
        fn.argtypes = argtypes
        fn.restype = ctypes.c_int
    got = lib.xw_abi_version()
    if got != ABI_VERSION:
        raise XnwanError('libxnwan.so ABI version %d, host expects %d -- rebuild' % (got, ABI_VERSION))
    return lib


lib = _load()


def check(status, what):
    if status == 0:
        return
    if status in ERRORS:
        buf = ctypes.create_string_buffer(512)
        lib.xw_supported_dims(buf, 512)
        raise XnwanError('%s: %s (compiled: %s)' % (what, ERRORS[status], buf.value.decode()))
    raise XnwanError('%s: HIP launch error %d' % (what, status))
