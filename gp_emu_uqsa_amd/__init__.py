"""gp_emu_uqsa_amd -- MI355X-native hot path of the GP_emu_UQSA Gaussian-process
emulator, behind the reference's API:

    import gp_emu_uqsa_amd as g
    E = g.setup("toy-sim_config")
    g.train(E)
    mean, var = g.posterior(E, x)

The covariance build, Cholesky factorisation, triangular solves, log-marginal-
likelihood gradient and posterior run in libgpemu.so (hand-written HIP for
gfx950, C-ABI in include/gpemu.h); there is no CPU fallback.
"""
from .api import (loo, plot, posterior, posterior_gradient, posterior_groups, posterior_mean,  # noqa: F401
                  posterior_sample, setup, train)
from . import multioutput  # noqa: F401  (p outputs with one correlation matrix: multioutput.setup / train / posterior)
from . import history_match  # noqa: F401  (imp_plot, nonimp_data, new_wave_design; EmulatorSet, implausibility, implausibility_mv, nonimp_sample)

__all__ = ["setup", "train", "plot", "posterior", "posterior_sample", "loo", "posterior_gradient",
           "posterior_mean", "posterior_groups", "multioutput", "history_match"]
__version__ = "0.1.0"
