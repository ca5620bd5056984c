"""ctypes binding of the C ABI in include/pigs_amd.h (pigs_amd/libpigs_amd.so).

There is no fallback: if the HIP library is missing or a call fails, an exception is raised.
"""
import ctypes
import os

# torch must be imported before libpigs_amd.so is loaded: both need libamdhip64, and the library
# must bind to the HIP runtime instance PyTorch brings along (loaded the other way round, the
# process holds two runtimes and ours reports "no ROCm-capable device").
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
# PIGS_AMD_LIB selects another build of the same ABI (kernel experiments); default: in-tree library
LIB_PATH = os.environ.get("PIGS_AMD_LIB") or os.path.join(HERE, "libpigs_amd.so")

PIGS_F32, PIGS_F64 = 0, 1
ABI_VERSION = 10

_vp = ctypes.c_void_p
_i = ctypes.c_int
_i64 = ctypes.c_int64
_ip = ctypes.POINTER(ctypes.c_int)          # a host array of ints
_vpp = ctypes.POINTER(ctypes.c_void_p)      # a host array of device pointers

DTYPES = {torch.float32: PIGS_F32, torch.float64: PIGS_F64}


def ptr(t):
    """The device pointer of a tensor; null for None and for an empty tensor."""
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() > 0 else ctypes.c_void_p(0)


def pointers(tensors):
    """A host array of device pointers; null for None."""
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() if t is not None else None for t in tensors])


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream(device):
    # the current stream's handle: the raw getter skips building a torch.cuda.Stream object (5 us a call)
    if _raw_stream is not None and device.index is not None:
        return ctypes.c_void_p(_raw_stream(device.index))
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class PigsResidualTerms(ctypes.Structure):
    """struct PigsResidualTerms of include/pigs_amd.h (the general residual's coefficients)"""
    _fields_ = [("a0", ctypes.c_double), ("a1", ctypes.c_double * 2), ("aL", ctypes.c_double), ("adv", ctypes.c_double),
                ("advect_by", (ctypes.c_double * 4) * 2),
                ("a0_pt", _vp), ("a1_pt", _vp), ("aL_pt", _vp), ("adv_pt", _vp)]


_terms_p = ctypes.POINTER(PigsResidualTerms)


class PigsResidualCoupling(ctypes.Structure):
    """struct PigsResidualCoupling of include/pigs_amd.h (the coupled residual's coefficients and matrices)"""
    _fields_ = [("a0", ctypes.c_double), ("aL", ctypes.c_double), ("cw", ctypes.c_double),
                ("couple0", (ctypes.c_double * 4) * 4), ("couple_lap", (ctypes.c_double * 4) * 4),
                ("a0_pt", _vp), ("aL_pt", _vp), ("cw_pt", _vp)]


_coupling_p = ctypes.POINTER(PigsResidualCoupling)


class PigsVorticityResidual(ctypes.Structure):
    """struct PigsVorticityResidual of include/pigs_amd.h (the vorticity residual's coefficients and tau field)"""
    _fields_ = [("nu", ctypes.c_double), ("dt", ctypes.c_double), ("time_term", ctypes.c_double), ("tau", ctypes.c_double),
                ("tau_pt", _vp)]


_vorticity_residual_p = ctypes.POINTER(PigsVorticityResidual)


class PigsVorticityFit(ctypes.Structure):
    """struct PigsVorticityFit of include/pigs_amd.h (the vorticity residual's coefficients, the data and its weight)"""
    _fields_ = [("nu", ctypes.c_double), ("dt", ctypes.c_double), ("time_term", ctypes.c_double), ("tau", ctypes.c_double),
                ("data_weight", ctypes.c_double), ("tau_pt", _vp), ("data", _vp)]


_vorticity_fit_p = ctypes.POINTER(PigsVorticityFit)


class PigsNetworkInputs(ctypes.Structure):
    """struct PigsNetworkInputs of include/pigs_amd.h (the right-hand side's kind, nu and the two wave constants)"""
    _fields_ = [("kind", _i), ("nu", ctypes.c_double), ("wave", ctypes.c_double * 2)]


_network_inputs_p = ctypes.POINTER(PigsNetworkInputs)


class PigsAdamStep(ctypes.Structure):
    """struct PigsAdamStep of include/pigs_amd.h (the optimiser's rates, running products and parameterisation)"""
    _fields_ = [("lr", ctypes.c_double * 4), ("beta1", ctypes.c_double), ("beta2", ctypes.c_double), ("eps", ctypes.c_double),
                ("beta1_pow", ctypes.c_double * 4), ("beta2_pow", ctypes.c_double * 4), ("scale", ctypes.c_double),
                ("wrap_lo", ctypes.c_double), ("wrap_hi", ctypes.c_double), ("means_map", _i), ("wrap", _i),
                ("device_lr", _vp), ("device_state", _vp)]


_adam_p = ctypes.POINTER(PigsAdamStep)


class PigsGradStats(ctypes.Structure):
    """struct PigsGradStats of include/pigs_amd.h (the optimiser's six statistic arrays and its device counts)"""
    _fields_ = [("mean_grad", _vp), ("mean_grad_norm", _vp), ("scale_grad", _vp), ("scale_grad_norm", _vp),
                ("last_mean_grad", _vp), ("last_scale_grad", _vp), ("device_counts", _vp)]


_stats_p = ctypes.POINTER(PigsGradStats)

NETWORK_ADAM_MAX_TENSORS = 128


class PigsNetworkAdam(ctypes.Structure):
    """struct PigsNetworkAdam of include/pigs_amd.h (the network optimiser's tensor table, its rates and its decay)"""
    _fields_ = [("tensors", _i), ("counts", _i64 * NETWORK_ADAM_MAX_TENSORS), ("params", _vp * NETWORK_ADAM_MAX_TENSORS),
                ("grads", _vp * NETWORK_ADAM_MAX_TENSORS), ("lr", ctypes.c_double), ("beta1", ctypes.c_double),
                ("beta2", ctypes.c_double), ("eps", ctypes.c_double), ("decay", ctypes.c_double), ("dev_lr", _vp)]


_network_adam_p = ctypes.POINTER(PigsNetworkAdam)

# name -> (restype, argtypes); must list every symbol include/pigs_amd.h declares
SIGNATURES = {
    "pigs_abi_version": (_i, []),
    "pigs_status_string": (ctypes.c_char_p, [_i]),
    "pigs_last_hip_error": (ctypes.c_char_p, []),
    "pigs_sample_forward": (_i, [_i, _i, _i, _i, _i64, _i64] + [_vp] * 4 + [_vp] * 4 + [_vp]),
    "pigs_sample_backward": (_i, [_i, _i, _i, _i, _i64, _i64] + [_vp] * 4 + [_vp] * 4 + [_vp] * 3 + [_vp]),
    "pigs_build_covariances": (_i, [_i, _i64] + [_vp] * 4 + [_vp]),
    "pigs_build_covariances_backward": (_i, [_i, _i64] + [_vp] * 6 + [_vp]),
    "pigs_samples_workspace_bytes": (ctypes.c_size_t, [_i64]),
    "pigs_plan_workspace_bytes": (ctypes.c_size_t, [_i64, _i64, _i]),
    "pigs_plan_layout_info": (_i, [_i64, _i64, _i, ctypes.POINTER(_i64)]),
    "pigs_samples_layout_info": (_i, [_i64, ctypes.POINTER(_i64)]),             # additive to ABI 10
    "pigs_plan_records_info": (_i, [_i64, _i64, _i, ctypes.POINTER(_i64)]),     # additive to ABI 10
    "pigs_samples_error_offset": (ctypes.c_size_t, []),
    "pigs_plan_error_offset": (ctypes.c_size_t, []),
    "pigs_samples_lattice_offset": (ctypes.c_size_t, []),
    "pigs_plan_strips_offset": (ctypes.c_size_t, []),
    "pigs_samples_build": (_i, [_vp, ctypes.c_size_t, _i64, _vp, _vp]),
    "pigs_samples_order_hint": (_i, [_i64]),
    "pigs_samples_trust_info": (_i, [_i64, ctypes.POINTER(_i64)]),              # additive to ABI 10
    "pigs_plan_build": (_i, [_vp, ctypes.c_size_t, _vp, ctypes.c_size_t, _i, _i64, _i64, _i, ctypes.c_float, ctypes.c_float]
                        + [_vp] * 4 + [_vp]),
    "pigs_plan_forward": (_i, [_vp, ctypes.c_size_t, _vp, ctypes.c_size_t, _i64, _i64, _i, ctypes.c_float, _i]
                          + [_vp] * 4 + [_vp]),
    "pigs_plan_backward": (_i, [_vp, ctypes.c_size_t, _vp, ctypes.c_size_t, _i64, _i64, _i, ctypes.c_float, _i]
                           + [_vp] * 4 + [_vp] * 3 + [_vp]),
    "pigs_residual_forward": (_i, [_i, _i, _i, _i64, _i64] + [_vp] * 4 + [ctypes.POINTER(ctypes.c_double), _vp, _vp]
                              + [_vp, ctypes.c_size_t, _vp, ctypes.c_size_t, _vp]),
    "pigs_residual_backward": (_i, [_i, _i, _i, _i64, _i64] + [_vp] * 4 + [ctypes.POINTER(ctypes.c_double), _vp] + [_vp] * 3
                               + [_vp, ctypes.c_size_t, _vp, ctypes.c_size_t, _vp]),
    # the general residual (additive to ABI 10): terms, target, out, aux / terms, gout, aux, gradients
    "pigs_residual_terms_forward": (_i, [_i, _i, _i, _i64, _i64] + [_vp] * 4 + [_terms_p, _vp, _vp, _vp]
                                    + [_vp, ctypes.c_size_t, _vp, ctypes.c_size_t, _vp]),
    "pigs_residual_terms_backward": (_i, [_i, _i, _i, _i64, _i64] + [_vp] * 4 + [_terms_p, _vp, _vp] + [_vp] * 3
                                     + [_vp, ctypes.c_size_t, _vp, ctypes.c_size_t, _vp]),
    # the vorticity terms (additive to ABI 10; d = 2, c = 2 implied): out [M][7] / gout [M][7], gradients
    "pigs_vorticity_forward": (_i, [_i, _i64, _i64] + [_vp] * 4 + [_vp] + [_vp, ctypes.c_size_t, _vp, ctypes.c_size_t, _vp]),
    "pigs_vorticity_backward": (_i, [_i, _i64, _i64] + [_vp] * 4 + [_vp] + [_vp] * 3
                                + [_vp, ctypes.c_size_t, _vp, ctypes.c_size_t, _vp]),
    # the vorticity residual (additive to ABI 10): params, prev, out, aux / params, gout, aux, gradients
    "pigs_vorticity_residual_forward": (_i, [_i, _i64, _i64] + [_vp] * 4 + [_vorticity_residual_p, _vp, _vp, _vp]
                                        + [_vp, ctypes.c_size_t, _vp, ctypes.c_size_t, _vp]),
    "pigs_vorticity_residual_backward": (_i, [_i, _i64, _i64] + [_vp] * 4 + [_vorticity_residual_p, _vp, _vp] + [_vp] * 3
                                         + [_vp, ctypes.c_size_t, _vp, ctypes.c_size_t, _vp]),
    # the vorticity fit (additive to ABI 10): the vorticity residual's arguments, out and gout [M][3]
    "pigs_vorticity_fit_forward": (_i, [_i, _i64, _i64] + [_vp] * 4 + [_vorticity_fit_p, _vp, _vp, _vp]
                                   + [_vp, ctypes.c_size_t, _vp, ctypes.c_size_t, _vp]),
    "pigs_vorticity_fit_backward": (_i, [_i, _i64, _i64] + [_vp] * 4 + [_vorticity_fit_p, _vp, _vp] + [_vp] * 3
                                    + [_vp, ctypes.c_size_t, _vp, ctypes.c_size_t, _vp]),
    # the image lookup (additive to ABI 10): dtypes, H, W, M, lo, hi, image, samples, out
    "pigs_grid_lookup": (_i, [_i, _i, _i64, _i64, _i64, ctypes.c_double, ctypes.c_double, _vp, _vp, _vp] + [_vp]),
    # the network inputs (additive to ABI 10; forward only): params, sample_u, sample_ux, sample_uxx, sample_pde
    "pigs_network_inputs_forward": (_i, [_i, _i, _i, _i64, _i64] + [_vp] * 4 + [_network_inputs_p] + [_vp] * 4
                                    + [_vp, ctypes.c_size_t, _vp, ctypes.c_size_t, _vp]),
    # the coupled residual (additive to ABI 10): coupling, target, out / coupling, gout, gradients
    "pigs_residual_coupled_forward": (_i, [_i, _i, _i, _i64, _i64] + [_vp] * 4 + [_coupling_p, _vp, _vp]
                                      + [_vp, ctypes.c_size_t, _vp, ctypes.c_size_t, _vp]),
    "pigs_residual_coupled_backward": (_i, [_i, _i, _i, _i64, _i64] + [_vp] * 4 + [_coupling_p, _vp] + [_vp] * 3
                                       + [_vp, ctypes.c_size_t, _vp, ctypes.c_size_t, _vp]),
    "pigs_periodic_images": (_i, [_i, _i, _i64, ctypes.c_double, ctypes.c_double, ctypes.c_double] + [_vp] * 6
                             + [_vp, _vp]),
    "pigs_periodic_images_backward": (_i, [_i, _i, _i64] + [_vp] * 6 + [_vp]),
    "pigs_aggregate_workspace_bytes": (ctypes.c_size_t, [_i, _i64]),
    "pigs_aggregate_lds_bytes": (ctypes.c_size_t, [_i, _i, _i, _i]),      # additive to ABI 10
    "pigs_aggregate_grid_info": (_i, [_i, _i64, ctypes.POINTER(_i64)]),     # additive to ABI 10
    "pigs_aggregate_lists": (_i, [_i, _i64, _i64, _vp, _vp, ctypes.c_double, _vp, ctypes.c_size_t, _i] + [_vp] * 5 + [_vp]),
    "pigs_aggregate_forward": (_i, [_i, _i64, _i64, _i, _i, _i] + [_vp] * 4 + [_vp] * 6 + [_vp] * 3 + [_vp]),
    "pigs_aggregate_backward_scratch_bytes": (ctypes.c_size_t, [_i, _i64, _i, _i]),
    "pigs_aggregate_backward": (_i, [_i, _i64, _i64, _i, _i, _i] + [_vp] * 6 + [_vp] * 6 + [_vp] * 3 + [_vp, ctypes.c_size_t]
                                + [_vp] * 6 + [_vp]),
    # the same on the torus of pigs_periodic_images (additive to ABI 10): + lo, period / + period
    "pigs_aggregate_lists_periodic": (_i, [_i, _i64, _i64, _vp, _vp, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                           _vp, ctypes.c_size_t, _i] + [_vp] * 5 + [_vp]),
    "pigs_aggregate_forward_periodic": (_i, [_i, _i64, _i64, _i, _i, _i, ctypes.c_double] + [_vp] * 4 + [_vp] * 6 + [_vp] * 3
                                        + [_vp]),
    "pigs_aggregate_backward_periodic": (_i, [_i, _i64, _i64, _i, _i, _i, ctypes.c_double] + [_vp] * 6 + [_vp] * 6 + [_vp] * 3
                                         + [_vp, ctypes.c_size_t] + [_vp] * 6 + [_vp]),
    # all heads of a layer in one launch (additive to ABI 10): + H, period (0 = plain lists)
    "pigs_aggregate_heads_lds_bytes": (ctypes.c_size_t, [_i, _i, _i, _i, _i]),
    "pigs_aggregate_heads_backward_scratch_bytes": (ctypes.c_size_t, [_i, _i64, _i, _i, _i]),
    "pigs_aggregate_heads_forward": (_i, [_i, _i64, _i64, _i, _i, _i, _i, ctypes.c_double] + [_vp] * 4 + [_vp] * 6 + [_vp] * 3
                                     + [_vp]),
    "pigs_aggregate_heads_backward": (_i, [_i, _i64, _i64, _i, _i, _i, _i, ctypes.c_double] + [_vp] * 6 + [_vp] * 6 + [_vp] * 3
                                      + [_vp, ctypes.c_size_t] + [_vp] * 6 + [_vp]),
    # refinement (additive to ABI 10): prune and split / clone Gaussians; masks, workspace, maps, counts / maps, arrays
    "pigs_refine_workspace_bytes": (ctypes.c_size_t, [_i64]),
    "pigs_refine_index": (_i, [_i, _i64, _vp, _vp, _vp, ctypes.c_size_t] + [_vp] * 3 + [_vp]),
    "pigs_refine_apply": (_i, [_i, _i, _i, _i64, _i64, ctypes.c_double] + [_vp] * 2 + [_vp] * 4 + [_vp] * 4 + [_vp] * 2
                          + [_vp]),
    "pigs_refine_backward": (_i, [_i, _i, _i, _i64, _i64, ctypes.c_double] + [_vp] * 2 + [_vp] * 4 + [_vp] * 4 + [_vp]),
    # the split criteria (additive to ABI 10): inputs, masks, workspace, metric / stats, mask
    "pigs_criterion_lds_values": (_i, []),
    "pigs_criterion_workspace_bytes": (ctypes.c_size_t, [_i, _i64, _i]),
    "pigs_criterion_quantile_mask": (_i, [_i, _i, _i, _i64, ctypes.c_double] + [_vp] * 4 + [_vp, ctypes.c_size_t]
                                     + [_vp] * 3 + [_vp]),
    "pigs_criterion_meanstd_mask": (_i, [_i, _i, _i64, ctypes.c_double] + [_vp] * 2 + [_vp, ctypes.c_size_t] + [_vp] * 2
                                    + [_vp]),
    # the optimiser (additive to ABI 10): parameters, outputs / hyper, parameters, moments, gradients, outputs
    "pigs_optim_materialize": (_i, [_i, _i, _i64, ctypes.c_double] + [_vp] * 3 + [_vp] * 3 + [_vp]),
    "pigs_optim_step": (_i, [_i, _i, _i64, _adam_p] + [_vp] * 4 + [_vp] * 8 + [_vp] * 4 + [_vp] * 3 + [_vp]),
    # its gradient statistics and its d = 1 form (additive to ABI 10): + stats / three groups, stats or NULL
    "pigs_optim_step_stats": (_i, [_i, _i, _i64, _adam_p] + [_vp] * 4 + [_vp] * 8 + [_vp] * 4 + [_vp] * 3 + [_stats_p, _vp]),
    "pigs_optim1d_materialize": (_i, [_i, _i, _i64, ctypes.c_double] + [_vp] * 2 + [_vp] * 3 + [_vp]),
    "pigs_optim1d_step": (_i, [_i, _i, _i64, _adam_p] + [_vp] * 3 + [_vp] * 6 + [_vp] * 4 + [_vp] * 3 + [_stats_p, _vp]),
    # the network's optimiser (additive to ABI 10): block, state, the flat moments, loss, its dtype
    "pigs_network_adam_state_doubles": (_i, [_i]),
    "pigs_network_adam_step": (_i, [_i, _network_adam_p, _vp, _vp, _vp, _vp, _i, _vp]),
    # the model's state update (additive to ABI 10): wrap, state, deltas, mask, scratch, the nine outputs /
    # saved arrays, mask, scratch, the nine incoming gradients, the five gradients
    "pigs_advance_scratch_bytes": (ctypes.c_size_t, [_i64]),
    "pigs_advance_forward": (_i, [_i, _i, _i64, _i, ctypes.c_double, ctypes.c_double] + [_vp] * 4 + [_vp, _vp]
                             + [_vp, ctypes.c_size_t] + [_vp] * 9 + [_vp]),
    "pigs_advance_backward": (_i, [_i, _i, _i64] + [_vp] * 3 + [_vp, _vp] + [_vp] * 9 + [_vp] * 5 + [_vp]),
    # the TEST problem's state terms (additive to ABI 10): wall, drift, means, u, deltas, mask, scratch, terms /
    # ..., scratch, g_terms, the three gradients
    "pigs_state_loss_scratch_bytes": (ctypes.c_size_t, [_i64]),
    "pigs_state_loss_forward": (_i, [_i, _i, _i64, ctypes.c_double, ctypes.c_double] + [_vp] * 3 + [_vp]
                                + [_vp, ctypes.c_size_t] + [_vp] + [_vp]),
    "pigs_state_loss_backward": (_i, [_i, _i, _i64, ctypes.c_double, ctypes.c_double] + [_vp] * 3 + [_vp] + [_vp, _vp]
                                 + [_vp] * 3 + [_vp]),
    # one tanh network per launch (additive to ABI 10): widths, x, weights, biases, y / ..., g_y, scratch, the gradients
    "pigs_mlp_scratch_bytes": (ctypes.c_size_t, [_i64, _i, _ip]),
    "pigs_mlp_forward": (_i, [_i, _i64, _i, _ip, _vp, _vpp, _vpp, _vp, _vp]),
    "pigs_mlp_backward": (_i, [_i, _i64, _i, _ip, _vp, _vpp, _vpp, _vp, _vp, ctypes.c_size_t, _vp, _vpp, _vpp, _vp]),
    # a bank of B nets of one shape over one x (additive to ABI 10): + B, G; the pointer arrays hold B * L entries
    "pigs_mlp_bank_scratch_bytes": (ctypes.c_size_t, [_i64, _i, _i, _ip]),
    "pigs_mlp_bank_forward": (_i, [_i, _i64, _i, _i, _i, _ip, _vp, _vpp, _vpp, _vp, _vp]),
    "pigs_mlp_bank_backward": (_i, [_i, _i64, _i, _i, _i, _ip, _vp, _vpp, _vpp, _vp, _vp, ctypes.c_size_t, _vp, _vpp, _vpp,
                                    _vp]),
    # one net over a row in P arrays, with block means (additive to ABI 10): widths, P, part_widths, parts, blocks, weights,
    # biases, scratch, y, m / ..., g_y, g_m, scratch, g_parts, the parameter gradients
    "pigs_mlp_joined_scratch_bytes": (ctypes.c_size_t, [_i64, _i, _ip, _i, _ip, _i]),
    "pigs_mlp_joined_forward": (_i, [_i, _i64, _i, _ip, _i, _ip, _vpp, _ip, _vpp, _vpp, _vp, ctypes.c_size_t, _vp, _vp, _vp]),
    "pigs_mlp_joined_backward": (_i, [_i, _i64, _i, _ip, _i, _ip, _vpp, _ip, _vpp, _vpp, _vp, _vp, _vp, ctypes.c_size_t, _vpp,
                                      _vpp, _vpp, _vp]),
    # the input transform (additive to ABI 10): dtype, N, c, p, the row arrays, ... ; params / g_params are 36 pointers
    "pigs_input_transform_scratch_bytes": (ctypes.c_size_t, [_i64, _i, _i]),
    "pigs_input_transform_matrices_forward": (_i, [_i, _i64, _i, _i] + [_vp] * 8 + [_vpp, _vp, ctypes.c_size_t, _vp, _vp, _vp]),
    "pigs_input_transform_matrices_backward": (_i, [_i, _i64, _i, _i] + [_vp] * 8 + [_vpp, _vp, _vp, _vp, ctypes.c_size_t]
                                               + [_vp] * 3 + [_vpp, _vp]),
    "pigs_input_transform_apply_forward": (_i, [_i, _i64, _i, _i] + [_vp] * 8 + [_vp, _vp]),
    "pigs_input_transform_apply_backward": (_i, [_i, _i64, _i, _i] + [_vp] * 7 + [_vp, _vp, ctypes.c_size_t] + [_vp] * 3 + [_vp]),
}

_lib = None


class PigsError(RuntimeError):
    pass


def load():
    """Load (once) and return the ctypes handle of libpigs_amd.so."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build the HIP library first (python -m pigs_amd.build). "
            "pigs_amd has no CPU or PyTorch fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise ImportError(f"{LIB_PATH} does not export {name}: it was built from older sources; rebuild "
                              "(python -m pigs_amd.build)") from None
        fn.restype = res
        fn.argtypes = args
    if lib.pigs_abi_version() != ABI_VERSION:
        raise ImportError(f"{LIB_PATH}: ABI version {lib.pigs_abi_version()} != {ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def check(status, what):
    if status != 0:
        lib = load()
        msg = lib.pigs_status_string(status).decode()
        if status == 3:
            msg += ": " + lib.pigs_last_hip_error().decode()
        raise PigsError(f"{what}: {msg} (status {status})")
