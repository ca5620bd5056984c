"""pigs_amd -- MI355X-native differentiable Gaussian sampler (the hot path of kr4b/pigs).

Public surface:
    GaussianSampler         drop-in for ``diff_gaussian_sampling.GaussianSampler``
    VORTICITY_COLUMNS       the column names of ``GaussianSampler.vorticity_terms()``
    VORTICITY_RESIDUAL_COLUMNS  the column names of ``GaussianSampler.vorticity_residual()``
    VORTICITY_FIT_COLUMNS   the column names of ``GaussianSampler.vorticity_residual(data=...)``
    grid_lookup             the pixel of an image under every sample point in one launch: the data of the reference's
                            vorticity fits (pigs_amd.lookup; main_pn.py:206-210, test_initialize.py:132-135)
    NETWORK_PDES            the right-hand sides ``GaussianSampler.network_inputs()`` composes
    covariances             fused ``build_covariances`` / ``build_full_covariances`` (gaussians.py:163-193)
    split_gaussians         prune and split / clone Gaussians in HIP with one host read (pigs_amd.refine;
                            model_pn.py:578-605, :703-714 and test_no_mlp.py:198-240)
    refine_index            its (source, child) maps alone, for optimiser state and other per-Gaussian arrays
    split_criterion         which Gaussians to split, as a mask on the device without a host wait: the sampling
                            passes and the quantile rule of model_pn.py:716-754 (pigs_amd.refine)
    split_mask              the quantile rule alone (:733-754), from the three sampled fields
    threshold_mask          score > mean + k std, the rule of test_no_mlp.py:203-205
    GaussianAdam            the Gaussians' parameterisation, its backward and Adam in one launch per step
                            (pigs_amd.optim; test_no_mlp.py:99-104, 146, 185-186, test_initialize.py:172-180); with
                            ``grad_stats=True`` also the densification's gradient sums (test_no_mlp.py:149-155)
    GaussianAdam1D          the same for d = 1 (test_no_mlp_1d.py:109-111, 156-162, 189-190)
    NetworkAdam             a drop-in for ``torch.optim.Adam(model.parameters())`` in the loop with the network: Adam over
                            up to 128 small tensors in two launches, the loss-weighted rate and the epoch's loss sums on
                            the device (pigs_amd.network_adam; main_pn.py:59, 157, 217-228)
    advance_gaussians       the dynamics network's deltas applied to the Gaussians, the next covariances and the
                            conservation penalty in two launches, one for the backward (pigs_amd.advance;
                            model_pn.py:270-273, 677-698, 878-882)
    ADVANCE_PENALTY_COLUMNS the names of ``advance_gaussians(...).penalty``'s four entries
    state_loss_terms        the eight state terms of Problem.TEST's pde, bc and conservation losses in one launch and one
                            for the backward, no host decision (pigs_amd.state_loss; model_pn.py:851-861, 866-876)
    STATE_LOSS_COLUMNS      the names of its eight entries
    fused_mlp               one per-Gaussian tanh network (nn.Linear layers with nn.Tanh between them, up to 6 layers
                            of width up to 48) in one launch forward and at most two backward, on the f32 MFMA
                            (pigs_amd.mlp; model_pn.py:154-174, 187-198, 203-226)
    FusedMLP                ``FusedMLP.from_sequential(seq)``: the same, as a module over an existing nn.Sequential
                            whose Parameters and state_dict keys it keeps
    fused_mlp_bank          up to 8 such nets of one shape over one input in one launch forward and at most two
                            backward; the model's query / key nets of all heads leave ``queries`` and ``keys`` in the
                            layout of ``aggregate_neighbors_heads`` (pigs_amd.mlp; model_pn.py:259-261)
    FusedMLPBank            ``FusedMLPBank(nets, groups)``: the same as a non-owning callable over existing nets
    fused_mlp_joined        such a net on a row that lies in up to 4 arrays, without the cat, and optionally the block means
                            of squares of those arrays: delta_net on (features, heads) and magnitude_loss's head
                            magnitudes; ``FusedMLP.joined`` is the same over a module (model_pn.py:265-268, 892-901)
    transform_matrices     the input transform's five matrices from the Gaussians (latent net, mean, five
                            TransformNets) in two launches (pigs_amd.input_transform; model_pn.py:51-119)
    apply_transforms        those matrices applied to the rows: ``t_params`` in one launch (model_pn.py:121-152, 237-249)
    FusedInputTransform     ``FusedInputTransform.from_module(m)``: both, as a module over an existing InputTransform
                            whose Parameters and state_dict keys it keeps
    build()                 compile the HIP library (hipcc, gfx950) and the native host extension in-tree
"""
from .build import build_all as build  # noqa: F401  (libpigs_amd.so + the native host extension)


def __getattr__(name):
    # lazy: importing the package must not require the built library (build() creates it)
    if name == "GaussianSampler":
        from .sampler import GaussianSampler
        return GaussianSampler
    if name == "VORTICITY_COLUMNS":
        from .sampler import VORTICITY_COLUMNS
        return VORTICITY_COLUMNS
    if name == "VORTICITY_RESIDUAL_COLUMNS":
        from .sampler import VORTICITY_RESIDUAL_COLUMNS
        return VORTICITY_RESIDUAL_COLUMNS
    if name == "VORTICITY_FIT_COLUMNS":
        from .sampler import VORTICITY_FIT_COLUMNS
        return VORTICITY_FIT_COLUMNS
    if name == "grid_lookup":
        from .lookup import grid_lookup
        return grid_lookup
    if name == "NETWORK_PDES":
        from .sampler import NETWORK_PDES
        return NETWORK_PDES
    if name in ("split_gaussians", "refine_index", "split_mask", "threshold_mask", "split_criterion"):
        from . import refine
        return getattr(refine, name)
    if name in ("GaussianAdam", "GaussianAdam1D"):
        from . import optim
        return getattr(optim, name)
    if name == "NetworkAdam":
        from .network_adam import NetworkAdam
        return NetworkAdam
    if name in ("advance_gaussians", "ADVANCE_PENALTY_COLUMNS"):
        from . import advance
        return getattr(advance, name)
    if name in ("state_loss_terms", "STATE_LOSS_COLUMNS"):
        from . import state_loss
        return getattr(state_loss, name)
    if name in ("fused_mlp", "FusedMLP", "fused_mlp_bank", "FusedMLPBank", "fused_mlp_joined"):
        from . import mlp
        return getattr(mlp, name)
    if name in ("transform_matrices", "apply_transforms", "FusedInputTransform"):
        from . import input_transform
        return getattr(input_transform, name)
    raise AttributeError(name)
