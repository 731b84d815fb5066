"""History matching with batched posteriors.

Mirrors gp_emu_uqsa.history_match (history_match/history_match.py,
_hmutilfunctions.py): imp_plot, imp_plot_recon, nonimp_data and new_wave_design keep
the reference's arguments, printed progress, RNG use (one optLatinHyperCube per input
pair or wave) and files (`<m>_IMP_<i>_<j>`, `<m>_ODP_<i>_<j>`, `nonimp_`/`noninp_`,
the wave design).

The difference is how posteriors are called:
- imp_plot: the reference builds one Posterior per grid cell and emulator
  (history_match.py:91-121) and forms each cell's full n x n variance for its diagonal.
  Here every cell of an input pair goes into ONE diagonal-variance posterior per emulator
  (grid^2 * n points), streamed through gpe_posterior.
- nonimp_data / new_wave_design: one posterior per emulator, diagonal only.

Implausibility I = |mean - z| / sqrt(var + var_extra). Per point, the maxno largest over
emulators are taken. Per cell, IMP is their minimum over points and ODP the fraction
below cm (:123-136).

Plots use today's matplotlib: `set_facecolor` and `adjustable='box'` replace the removed
`set_axis_bgcolor` and `'box-forced'` of _hmutilfunctions.py:81,102.
"""
from __future__ import annotations

import numpy as _np

from . import design_inputs as _gd
from . import model as _model
from . import multioutput as _mo

__all__ = ["imp_plot", "imp_plot_recon", "nonimp_data", "new_wave_design", "EmulatorSet", "implausibility",
           "implausibility_mv", "nonimp_sample", "imp_maps"]


# ----------------------------------------------------------------- helpers (_hmutilfunctions.py)
def make_sets(ai):
    sets = []
    for i in ai:
        for j in ai:
            if i != j and i < j and [i, j] not in sets:
                sets.append([i, j])
    return sets


def emulsetup(emuls):
    minmax, orig_minmax = {}, {}
    sets = []
    for e in emuls:
        try:
            ai = e.beliefs.active_index
            mm = e.beliefs.input_minmax
        except AttributeError:
            print("ERROR: Emulator(s) were not previously trained and reconstructed "
                  "using updated beliefs files, "
                  "so they are missing 'active_index' and 'input_minmax'. Exiting.")
            raise SystemExit
        sets = make_sets(ai)
        for i in range(len(ai)):
            minmax[str(ai[i])] = list((_np.array(mm[i]) - mm[i][0]) / (mm[i][1] - mm[i][0]))
            orig_minmax[str(ai[i])] = list(_np.array(mm[i]))
    print("\nactive index pairs:", sets)
    print("\nminmax for active inputs:", minmax)
    print("original units minmax for active inputs:", orig_minmax)
    return sets, minmax, orig_minmax


def ref_act(minmax):
    act_ref = {key: c for c, key in enumerate(sorted(minmax.keys(), key=lambda x: int(x)))}
    print("\nrelate active_indices to integers:", act_ref)
    return act_ref


def ref_plt(act):
    plt_ref = {str(key): c for c, key in enumerate(sorted(act))}
    print("\nrelate restricted active_indices to subplot indices:", plt_ref)
    return plt_ref


def check_act(act, sets):
    if type(act) is not list:
        print("ERROR: 'act' argument must be a list, but", act, "was supplied. Exiting.")
        raise SystemExit
    flat = [item for sublist in sets for item in sublist]
    for a in act:
        if a not in flat:
            print("ERROR: index", a, "in 'act' is not an active_index of the emulator(s). Exiting.")
            raise SystemExit
    return True


def load_datafiles(datafiles, orig_minmax):
    try:
        sim_x, sim_y = _np.loadtxt(datafiles[0]), _np.loadtxt(datafiles[1])
    except FileNotFoundError:
        print("ERROR: datafile(s)", datafiles, "for inputs and/or outputs not found. Exiting.")
        raise SystemExit
    for key in orig_minmax.keys():
        sim_x[:, int(key)] = (sim_x[:, int(key)] - orig_minmax[key][0]) \
            / (orig_minmax[key][1] - orig_minmax[key][0])
    return sim_x, sim_y


def _posterior_diag(E, x_active):
    """Posterior mean and variance diagonal of emulator E at points x (its active
    inputs, scaled), one batched GPU call (reference: Data + Posterior per call site)."""
    ni = _model.Data(x_active, None, E.basis, E.par, E.beliefs, E.K)
    post = _model.Posterior(ni, E.training, E.par, E.beliefs, E.K, predict=True, full_var=False)
    return post.mean, post.var


def _imaxes(I2, maxno):
    """Per point, the maxno largest implausibilities over emulators, ascending."""
    I = _np.sqrt(I2)
    return _np.sort(_np.partition(I, -maxno, axis=1)[:, -maxno:], axis=1)


# ----------------------------------------------------------------- plotting
def make_plots(s, plt_ref, cm, maxno, ax, IMP, ODP, minmax=None, recon=False):
    import matplotlib.pyplot as _plt
    imp_pal = _plt.get_cmap('jet')
    odp_pal = _plt.get_cmap('afmhot')
    (odp, imp) = (ODP, IMP) if recon else (ODP[maxno - 1], IMP[maxno - 1])
    ax[plt_ref[str(s[0])], plt_ref[str(s[1])]].set_facecolor('darkgray')
    ex = None if recon else (minmax[str(s[0])][0], minmax[str(s[0])][1],
                             minmax[str(s[1])][0], minmax[str(s[1])][1])
    im_imp = ax[plt_ref[str(s[1])], plt_ref[str(s[0])]].imshow(
        imp.T, origin='lower', cmap=imp_pal, extent=ex, vmin=0.0, vmax=cm + 1, interpolation='none')
    im_odp = ax[plt_ref[str(s[0])], plt_ref[str(s[1])]].imshow(
        _np.ma.masked_where(odp == 0, odp).T, origin='lower', cmap=odp_pal, extent=ex, vmin=0.0,
        vmax=1.0, interpolation='none')
    _plt.colorbar(im_imp, ax=ax[plt_ref[str(s[1])], plt_ref[str(s[0])]])
    _plt.colorbar(im_odp, ax=ax[plt_ref[str(s[0])], plt_ref[str(s[1])]])


def plot_options(plt_ref, ax, fig, minmax=None):
    import matplotlib.pyplot as _plt
    for key in plt_ref:
        ax[plt_ref[key], plt_ref[key]].set(adjustable='box', aspect='equal')
        if minmax is not None:
            ax[plt_ref[key], plt_ref[key]].text(.25, .5, "Input " + str(key) + "\n"
                                                + str(minmax[key][0]) + "\n-\n" + str(minmax[key][1]))
        fig.delaxes(ax[plt_ref[key], plt_ref[key]])
    for a in ax.flat:
        a.set_xticks([])
        a.set_yticks([])
        a.set_aspect('equal')
    _plt.tight_layout()


def _save_maps(fileStr, s, maxno, IMP, ODP):
    nfileStr = fileStr + "_" if fileStr != "" else fileStr
    for m in range(maxno):
        _np.savetxt(nfileStr + str(m + 1) + "_" + "IMP_" + str(s[0]) + '_' + str(s[1]), IMP[m])
        _np.savetxt(nfileStr + str(m + 1) + "_" + "ODP_" + str(s[0]) + '_' + str(s[1]), ODP[m])


# ----------------------------------------------------------------- API (history_match.py)
def imp_plot(emuls, zs, cm, var_extra, maxno=1, olhcmult=100, grid=10, act=[], fileStr="", plot=True):
    """Implausibility (lower triangle) and optical depth (upper triangle) per pair of
    active inputs over a grid x grid mesh, each cell sampled by an oLHC design of the
    other inputs (reference :7-150).  Writes <m>_IMP_<i>_<j> / <m>_ODP_<i>_<j>.

    ``emuls`` may be an ``EmulatorSet``: every pair's maps then come from ``EmulatorSet.maps``
    (on a fused set: candidates made and reduced on the device), with the same
    optLatinHyperCube call per pair, the same prints and the same files.  A list keeps the
    ``_posterior_diag`` route below."""
    hset = emuls if isinstance(emuls, EmulatorSet) else None
    if hset is not None:
        emuls = hset._views
    sets, minmax, orig_minmax = emulsetup(emuls)
    check_act(act, sets)
    act_ref = ref_act(minmax)
    plt_ref = ref_plt(act)
    num_inputs = len(minmax)
    dim = num_inputs - 2
    maxno = int(maxno)
    IMP = [_np.zeros((grid, grid)) for _ in range(maxno)]
    ODP = [_np.zeros((grid, grid)) for _ in range(maxno)]
    print("Creating plot objects... may take some time...")
    plot = plot is True
    rc = num_inputs if act == [] else len(act)
    fig = ax = None
    if plot:
        import matplotlib.pyplot as _plt
        fig, ax = _plt.subplots(nrows=rc, ncols=rc)
    plt_ref = act_ref if act == [] else ref_plt(act)
    less_sets = sets if act == [] else [s for s in sets if s[0] in act and s[1] in act]
    print("HM for input pairs:", less_sets)

    for s in less_sets:
        print("\nset:", s)
        X1 = _np.linspace(minmax[str(s[0])][0], minmax[str(s[0])][1], grid, endpoint=False)
        X1 = X1 + 0.5 * (minmax[str(s[0])][1] - minmax[str(s[0])][0]) / float(grid)
        X2 = _np.linspace(minmax[str(s[1])][0], minmax[str(s[1])][1], grid, endpoint=False)
        X2 = X2 + 0.5 * (minmax[str(s[1])][1] - minmax[str(s[1])][0]) / float(grid)
        print("Values of the grid 1:", X1)
        print("Values of the grid 2:", X2)
        n = dim * int(olhcmult)
        N = int(n / 2)
        olhc_range = [it[1] for it in sorted(minmax.items(), key=lambda x: int(x[0]))
                      if int(it[0]) != s[0] and int(it[0]) != s[1]]
        print("olhc_range:", olhc_range)
        filename = "imp_input_" + str(s[0]) + '_' + str(s[1])
        _gd.optLatinHyperCube(dim, n, N, olhc_range, filename)
        x_other = _np.loadtxt(filename)
        if hset is not None:
            xo = x_other.reshape(n, -1) if x_other.ndim > 1 else x_other.reshape(n, 1)
            print("\nCalculating Implausibilities...")
            imp, odp = hset.maps(zs, var_extra, cm, (act_ref[str(s[0])], act_ref[str(s[1])]), X1, X2, xo,
                                 maxno=maxno, use=hset.pair_flags(s))
            for m in range(maxno):
                IMP[m][:, :] = imp[m]
                ODP[m][:, :] = odp[m]
            _save_maps(fileStr, s, maxno, IMP, ODP)
            if plot:
                make_plots(s, plt_ref, cm, maxno, ax, IMP, ODP, minmax=minmax)
            continue
        # every grid cell at once: cell c = i*grid + j owns rows [c n, (c+1) n)
        cells = grid * grid
        x = _np.empty((cells * n, num_inputs))
        c0 = _np.repeat(_np.repeat(X1, grid), n)
        c1 = _np.repeat(_np.tile(X2, grid), n)
        x[:, act_ref[str(s[0])]] = c0
        x[:, act_ref[str(s[1])]] = c1
        other_dim = [act_ref[str(key)] for key in act_ref if int(key) not in s]
        xo = x_other.reshape(n, -1) if x_other.ndim > 1 else x_other.reshape(n, 1)
        x[:, other_dim] = _np.tile(xo, (cells, 1))
        print("\nCalculating Implausibilities...")
        I2 = _np.zeros((cells * n, len(emuls)))
        for o in range(len(emuls)):
            E, z, var_e = emuls[o], zs[o], var_extra[o]
            Eai = E.beliefs.active_index
            if s[0] in Eai and s[1] in Eai:
                act_ind_list = [act_ref[str(l)] for l in Eai]
                mean, var = _posterior_diag(E, x[:, act_ind_list])
                I2[:, o] = (mean - z) ** 2 / (var + var_e)
        Imaxes = _imaxes(I2, maxno).reshape(cells, n, maxno)
        for m in range(maxno):
            col = Imaxes[:, :, -(m + 1)]
            IMP[m][:, :] = col.min(axis=1).reshape(grid, grid)
            ODP[m][:, :] = (col < cm).sum(axis=1).reshape(grid, grid) / float(n)
        _save_maps(fileStr, s, maxno, IMP, ODP)
        if plot:
            make_plots(s, plt_ref, cm, maxno, ax, IMP, ODP, minmax=minmax)
    if plot:
        import matplotlib.pyplot as _plt
        plot_options(plt_ref, ax, fig, minmax)
        _plt.show()
    return


def imp_plot_recon(cm, maxno=1, act=[], fileStr=""):
    """Re-plot from the files imp_plot wrote (reference :153-192)."""
    if act == []:
        print("WARNING: Please specificy 'act' for active inputs. Return None.")
        return None
    import matplotlib.pyplot as _plt
    print("Creating plot objects... may take some time...")
    fig, ax = _plt.subplots(nrows=len(act), ncols=len(act))
    plt_ref = ref_plt(act)
    sets = make_sets(act)
    print("HM for input pairs:", sets)
    for s in sets:
        print("\nset:", s)
        nfileStr = fileStr + "_" if fileStr != "" else fileStr
        IMP = _np.loadtxt(nfileStr + str(maxno) + "_" + "IMP_" + str(s[0]) + '_' + str(s[1]))
        ODP = _np.loadtxt(nfileStr + str(maxno) + "_" + "ODP_" + str(s[0]) + '_' + str(s[1]))
        make_plots(s, plt_ref, cm, maxno, ax, IMP, ODP, recon=True)
    plot_options(plt_ref, ax, fig)
    _plt.show()
    return


def _implausible_rows(emuls, zs, var_extra, x, act_ref, maxno, cm):
    if isinstance(emuls, EmulatorSet):
        return emuls.implausibility(zs, var_extra, x, maxno)[:, -maxno] < cm
    I2 = _np.zeros((x.shape[0], len(emuls)))
    for o in range(len(emuls)):
        E, z, var_e = emuls[o], zs[o], var_extra[o]
        act_ind_list = [act_ref[str(l)] for l in E.beliefs.active_index]
        mean, var = _posterior_diag(E, x[:, act_ind_list])
        I2[:, o] = (mean - z) ** 2 / (var + var_e)
    Imaxes = _imaxes(I2, maxno)
    return Imaxes[:, -maxno] < cm


def nonimp_data(emuls, zs, cm, var_extra, datafiles, maxno=1, act=[], fileStr=""):
    """Keep the non-implausible rows of a data set (reference :195-256).  Writes
    `nonimp_<inputs file>` (scaled inputs, as the reference) and `noninp_<outputs file>`.
    ``emuls``: a list (the ``_posterior_diag`` loop) or an ``EmulatorSet`` (its ``implausibility``)."""
    sets, minmax, orig_minmax = emulsetup(emuls._views if isinstance(emuls, EmulatorSet) else emuls)
    act_ref = ref_act(minmax)
    check_act(act, sets)
    maxno = int(maxno)
    sim_x, sim_y = load_datafiles(datafiles, orig_minmax)
    print("\nCalculating Implausibilities...")
    keep = _implausible_rows(emuls, zs, var_extra, sim_x, act_ref, maxno, cm)
    nimp_inputs, nimp_outputs = sim_x[keep], sim_y[keep]
    nfileStr = fileStr + "_" if fileStr != "" else fileStr
    _np.savetxt(nfileStr + "nonimp_" + datafiles[0], nimp_inputs)
    _np.savetxt(nfileStr + "noninp_" + datafiles[1], nimp_outputs)
    print(len(nimp_inputs), "data points were non-implausible")
    return len(nimp_inputs)


def new_wave_design(emuls, zs, cm, var_extra, datafiles, maxno=1, olhcmult=100, act=[], fileStr=""):
    """Non-implausible points of a new oLHC design optimised against the given
    (non-implausible) data (reference :259-339).  Writes `<fileStr_><inputs file>`.
    ``emuls``: a list or an ``EmulatorSet``, as ``nonimp_data``."""
    sets, minmax, orig_minmax = emulsetup(emuls._views if isinstance(emuls, EmulatorSet) else emuls)
    act_ref = ref_act(minmax)
    check_act(act, sets)
    dim = len(minmax)
    maxno = int(maxno)
    sim_x, sim_y = load_datafiles(datafiles, orig_minmax)
    n = dim * int(olhcmult)
    N = int(n / 2)
    olhc_range = [it[1] for it in sorted(minmax.items(), key=lambda x: int(x[0]))]
    print("olhc_range:", olhc_range)
    filename = "olhc_des"
    _gd.optLatinHyperCube(dim, n, N, olhc_range, filename, fextra=sim_x)
    x = _np.loadtxt(filename)
    if x.ndim == 1:
        x = x.reshape(-1, 1)
    print("\nCalculating Implausibilities...")
    keep = _implausible_rows(emuls, zs, var_extra, x, act_ref, maxno, cm)
    nimp_inputs = x[keep]
    nfileStr = fileStr + "_" if fileStr != "" else fileStr
    _np.savetxt(nfileStr + datafiles[0], nimp_inputs)
    print("Generated", len(nimp_inputs), "new data points")
    return len(nimp_inputs)


# ----------------------------------------------------------------- resident emulator set
class EmulatorSet:
    """The emulators of a wave resident on the GPU together (native.EmulatorSet, gpe_hm).

    Each emulator's training set is uploaded and factored once, as ``Sensitivity._gpu`` does,
    and snapshotted into the set; ``implausibility`` then runs any number of candidate points
    through all of them, one fused kernel per emulator and chunk.  ``fused`` is False when an
    emulator falls outside that path -- the library refuses it (n > 512, more than 32 inputs,
    16 basis columns or 32 emulators), a basis expression is neither the constant nor ``x``,
    or ``model.Posterior`` would add a host-side term to its variance -- and the whole set then
    computes through the ``_posterior_diag`` loop, with that loop's results.

    An item may be a trained ``multioutput.MultiEmulator``: one member of the set with one copy
    of L^-1 for its p outputs (gpe_hm_add_multi), which take p consecutive places in ``zs`` and
    ``var_extra``; output a has variance Sigma[a, a] c(x).  The limits then count outputs (32 per
    set, p + q <= 32 per item), and the route outside the fused path is
    ``multioutput.posterior``.  Where its beliefs carry no ``active_index`` / ``input_minmax``
    (``multioutput.train`` writes no beliefs file) the active inputs are ``beliefs.active``
    (``[]``: all) and the ranges ``all_data.input_minmax``.  ``implausibility_mv`` is the joint
    measure of such an item."""

    def __init__(self, emuls):
        self.emuls = list(emuls)
        self._multi = [isinstance(E, _mo.MultiEmulator) for E in self.emuls]
        for E, multi in zip(self.emuls, self._multi):
            if multi and E.Sigma is None:
                raise RuntimeError("train() the MultiEmulator first")
        views = [self._multi_view(E) if multi else E for E, multi in zip(self.emuls, self._multi)]
        _, minmax, _ = emulsetup(views)
        self.minmax = minmax
        self.act_ref = ref_act(minmax)
        self.D = len(minmax)
        self._views = views
        self._active = [list(E.beliefs.active_index) for E in views]
        self._cols = [[self.act_ref[str(l)] for l in E.beliefs.active_index] for E in views]
        # the items' places among the outputs: item i owns [_first[i], _first[i] + its outputs)
        counts = [E.p if multi else 1 for E, multi in zip(self.emuls, self._multi)]
        self._first = [int(v) for v in _np.concatenate([[0], _np.cumsum(counts)[:-1]])] if counts else []
        self.outputs = int(sum(counts))
        self._set = None
        self.fused = self._make_fused()

    @staticmethod
    def _multi_view(M):
        """What emulsetup reads of an item, for a MultiEmulator: its beliefs' ``active_index`` and
        ``input_minmax`` where a beliefs file gave them, else ``beliefs.active`` (all inputs
        when empty) and the ranges its inputs were scaled by."""
        from types import SimpleNamespace
        d = M.training.inputs.shape[1]
        ai = getattr(M.beliefs, "active_index", None)
        if not isinstance(ai, list) or len(ai) != d:
            ai = list(M.beliefs.active) if M.beliefs.active != [] else list(range(d))
        mm = M.beliefs.input_minmax
        if mm is None or len(mm) != d:
            mm = M.all_data.input_minmax
        if mm is None or len(mm) != d:
            mm = M.all_data.minmax
        mm = [[float(a), float(b)] for a, b in mm]
        return SimpleNamespace(beliefs=SimpleNamespace(active_index=[int(i) for i in ai], input_minmax=mm))

    @staticmethod
    def _basis_forms(E):
        """(hdim, hval) of E's basis if every column is the constant or the identity on one
        input (the reference's default mean functions), else None."""
        exprs = [str(e).strip() for e in E.beliefs.basis_str]
        if len(exprs) != len(E.basis.h) or any(e != "x" for e in exprs[1:]) \
                or any(str(e).strip() != "x" for e in E.basis.exprs[1:]):
            return None
        try:
            const = float(E.basis.h[0](1.0))
        except Exception:
            return None
        hdim = [-1] + [int(E.basis.basis_inf[j - 1]) for j in range(1, len(exprs))]
        return hdim, [const] + [0.0] * (len(exprs) - 1)

    @staticmethod
    def _host_var_term(E):
        """True if model.Posterior adds a term to the variance of new points on the host."""
        probe = _model.Data(_np.asarray(E.training.inputs)[:1], None, E.basis, E.par, E.beliefs, E.K)
        return probe.r_scale() != 0.0

    def _make_fused(self):
        from . import native as _native
        forms = [self._basis_forms(E) for E in self.emuls]
        if any(f is None for f in forms) or any(self._host_var_term(E) for E in self.emuls):
            return False
        nset = None
        try:
            for E, multi, cols, (hdim, hval) in zip(self.emuls, self._multi, self._cols, forms):
                if multi:
                    ctx = _mo._resident(E)
                else:
                    ctx = _model.upload_training(E.training)
                    ctx.ensure_factor(E.K.kind, E.K.d, float(E.K.n), 1.0, E.training.r_scale())
                if nset is None:
                    nset = _native.EmulatorSet(ctx.device)
                if multi:
                    nset.add_multi(ctx, cols, hdim, hval, E.B, E.Sigma)
                else:
                    nset.add(ctx, cols, hdim, hval, E.par.beta, float(E.par.sigma))
        except RuntimeError as err:
            if nset is not None:
                nset.close()
            if getattr(err, "status", None) == -5:   # GPE_ERR_UNSUPPORTED: beyond the set's limits
                return False
            raise
        self._set = nset
        return True

    def implausibility(self, zs, var_extra, x, maxno=1):
        """m x maxno: per point of x (m x D, scaled) the maxno largest implausibilities over
        the emulators, ascending."""
        x = _np.ascontiguousarray(x, dtype=float)
        if x.ndim == 1:
            x = x.reshape(-1, 1)
        maxno = int(maxno)
        if self.fused:
            return self._set.implausibility(x, zs, var_extra, maxno=maxno)
        return _imaxes(self._loop_i2(zs, var_extra, x), maxno)

    def _loop_i2(self, zs, var_extra, x, use=None):
        """I^2 (m x outputs) by the route outside the fused path; an item whose flag of ``use``
        (one per item) is off keeps its zero columns, as imp_plot's loop leaves them."""
        I2 = _np.zeros((x.shape[0], self.outputs))
        for i, (E, multi, cols, o) in enumerate(zip(self.emuls, self._multi, self._cols, self._first)):
            if use is not None and not use[i]:
                continue
            if multi:
                mean, c, Sigma = _mo.posterior(E, x[:, cols])
                for a in range(E.p):
                    I2[:, o + a] = (mean[:, a] - zs[o + a]) ** 2 / (Sigma[a, a] * c + var_extra[o + a])
            else:
                mean, var = _posterior_diag(E, x[:, cols])
                I2[:, o] = (mean - zs[o]) ** 2 / (var + var_extra[o])
        return I2

    def pair_flags(self, s):
        """imp_plot's rule for the input pair s = [i, j] (active indices): one flag per item, on
        where the item reads both inputs."""
        return [s[0] in ai and s[1] in ai for ai in self._active]

    def maps(self, zs, var_extra, cm, pair, x1, x2, others, maxno=1, use=None, joint=None):
        """The maps of imp_plot over the mesh x1 x x2 of the columns ``pair`` = (ca, cb) of the
        D-wide rows: (IMP, ODP), each maxno x g1 x g2.  Cell (i, j) has the ns candidates with
        x1[i] in column ca, x2[j] in column cb and ``others`` (ns x (D - 2)) in the remaining
        columns in ascending order.  Level l is the (l + 1)-th largest implausibility over the
        outputs (``Imaxes[:, :, -(l + 1)]`` of imp_plot); IMP is its minimum over a cell's
        candidates (NaN if one is NaN), ODP the fraction of them below cm.  ``use``: one flag per
        item (None: all on); an item switched off enters with I^2 = 0, imp_plot's untouched
        column.  ``joint`` = (item, V): the joint measure of that MultiEmulator in place of the
        univariate ones, one level; zs is then the item's z.

        A fused set makes the candidates and reduces them on the device (gpe_hm_cells): only
        the maps come back.  Any other set forms the explicit rows and reduces in NumPy."""
        ca, cb = int(pair[0]), int(pair[1])
        x1, x2 = _np.asarray(x1, dtype=float).ravel(), _np.asarray(x2, dtype=float).ravel()
        others = _np.asarray(others, dtype=float)
        if others.ndim == 1:
            others = others.reshape(-1, 1) if self.D != 2 else _np.zeros((others.size, 0))
        ns, maxno = others.shape[0], int(maxno)
        if joint is not None:
            item, V = int(joint[0]), _np.asarray(joint[1], dtype=float)
            if not 0 <= item < len(self.emuls) or not self._multi[item]:
                raise ValueError("joint takes an item that is a MultiEmulator")
            if V.ndim == 1:
                V = _np.diag(V)
            maxno = 1
        if self.fused:
            if joint is not None:
                imp, below = self._set.cells_mv(item, self.D, (ca, cb), x1, x2, others, zs, V, cm)
                imp, below = imp[None], below[None]
            else:
                flags = None
                if use is not None:
                    counts = [E.p if multi else 1 for E, multi in zip(self.emuls, self._multi)]
                    flags = _np.repeat(_np.asarray(use, dtype=bool), counts)
                imp, below = self._set.cells(self.D, (ca, cb), x1, x2, others, zs, var_extra, cm, maxno=maxno,
                                             use=flags)
            return imp, below / float(ns)
        g1, g2 = x1.size, x2.size
        cells = g1 * g2
        x = _np.empty((cells * ns, self.D))
        x[:, ca] = _np.repeat(_np.repeat(x1, g2), ns)
        x[:, cb] = _np.repeat(_np.tile(x2, g1), ns)
        x[:, [k for k in range(self.D) if k not in (ca, cb)]] = _np.tile(others, (cells, 1))
        if joint is not None:
            top = self.implausibility_mv(item, zs, V, x).reshape(-1, 1)
        elif use is None:
            top = self.implausibility(zs, var_extra, x, maxno)
        else:
            top = _imaxes(self._loop_i2(zs, var_extra, x, use), maxno)
        top = top.reshape(cells, ns, maxno)
        IMP, ODP = _np.empty((maxno, g1, g2)), _np.empty((maxno, g1, g2))
        for l in range(maxno):
            col = top[:, :, -(l + 1)]
            IMP[l] = col.min(axis=1).reshape(g1, g2)
            ODP[l] = (col < cm).sum(axis=1).reshape(g1, g2) / float(ns)
        return IMP, ODP

    def implausibility_mv(self, item, z, V, x, parts=False):
        """The joint (multivariate) implausibility of item ``item``, a MultiEmulator of p outputs,
        at the m points of x (m x D, scaled):

            I(x) = sqrt((z - mean(x))^T (c(x) Sigma + V)^-1 (z - mean(x)))

        with Sigma the between-output covariance, c the emulator's variance at sigma = 1 and V
        (p x p, or a length-p vector of variances: its diagonal) the observation error plus the
        model discrepancy (Vernon, Goldstein & Bower 2010).  The usual cut-off compares I^2 with
        a quantile of chi^2 with p degrees of freedom (0.995: 7.88 at p = 1, 10.6 at p = 2, 21.95
        at p = 8) where the maximum of univariate measures is compared with 3.  ``parts``: also
        the mean (m x p) and c (m)."""
        item = int(item)
        if not 0 <= item < len(self.emuls) or not self._multi[item]:
            raise ValueError("implausibility_mv takes an item that is a MultiEmulator")
        M, cols = self.emuls[item], self._cols[item]
        x = _np.ascontiguousarray(x, dtype=float)
        if x.ndim == 1:
            x = x.reshape(-1, 1)
        z = _np.asarray(z, dtype=float).ravel()
        V = _np.asarray(V, dtype=float)
        if V.ndim == 1:
            V = _np.diag(V)
        if z.size != M.p or V.shape != (M.p, M.p):
            raise ValueError("z has one entry per output of the item, and V is p x p (or its diagonal)")
        if self.fused:
            I2, mean, c = self._set.implausibility_mv(item, x, z, V, parts=True)
            mean = _np.ascontiguousarray(mean.T)
        else:
            mean, c, Sigma = _mo.posterior(M, x[:, cols])
            r = mean - z
            A = c[:, None, None] * Sigma[None, :, :] + V[None, :, :]
            I2 = _np.einsum("sa,sa->s", r, _np.linalg.solve(A, r[:, :, None])[:, :, 0])
        I = _np.sqrt(I2)
        return (I, mean, c) if parts else I

    def close(self):
        if self._set is not None:
            self._set.close()
            self._set = None
            self.fused = False


def _as_set(emuls_or_set):
    if isinstance(emuls_or_set, EmulatorSet):
        return emuls_or_set, False
    if isinstance(emuls_or_set, _mo.MultiEmulator):
        return EmulatorSet([emuls_or_set]), True
    return EmulatorSet(emuls_or_set), True


def implausibility_mv(M_or_set, z, V, x, item=0, parts=False):
    """The joint implausibility of a ``MultiEmulator`` (or of item ``item`` of a list or an
    ``EmulatorSet``) at every point of x: ``EmulatorSet.implausibility_mv``."""
    S, mine = _as_set(M_or_set)
    try:
        return S.implausibility_mv(item, z, V, x, parts)
    finally:
        if mine:
            S.close()


def implausibility(emuls_or_set, zs, var_extra, x, maxno=1):
    """The maxno largest implausibilities over the emulators at every point of x (m x D in the
    scaled inputs, one column per active input in ascending order): m x maxno, ascending, so
    column -maxno is what ``nonimp_data`` compares with the cut-off.  Takes a list of emulators
    or an ``EmulatorSet`` (kept resident between calls)."""
    S, mine = _as_set(emuls_or_set)
    try:
        return S.implausibility(zs, var_extra, x, maxno)
    finally:
        if mine:
            S.close()


def imp_maps(emuls_or_set, zs, var_extra, cm, pair, x1, x2, others, maxno=1, use=None, joint=None):
    """(IMP, ODP), each maxno x g1 x g2: imp_plot's two maps over the mesh x1 x x2 of the columns
    ``pair`` of the scaled D-wide rows, ``others`` (ns x (D - 2)) sampling every cell:
    ``EmulatorSet.maps``.  Takes a list of emulators or an ``EmulatorSet``."""
    S, mine = _as_set(emuls_or_set)
    try:
        return S.maps(zs, var_extra, cm, pair, x1, x2, others, maxno=maxno, use=use, joint=joint)
    finally:
        if mine:
            S.close()


def nonimp_sample(emuls_or_set, zs, cm, var_extra, count, maxno=1, seed=0, batch=2 ** 20, max_tried=None,
                  generator=None):
    """Rejection sampling of the non-implausible region: uniform candidates in the scaled box,
    ``np.random.default_rng(seed).random((batch, D))`` batch after batch, kept where the
    maxno-th largest implausibility is below cm.  Returns (points, tried): the first ``count``
    accepted candidates in stream order (fewer if ``max_tried`` candidates did not yield them)
    and the number of candidates drawn up to and including the last one returned, or all that
    were tried if fewer than ``count`` were found.  The result does not depend on ``batch``.

    ``generator``: ``"host"`` draws and maps the candidates in NumPy and uploads them;
    ``"device"`` (a fused set) reproduces the same PCG64 stream in a kernel from the generator's
    state and increment, so that nothing is uploaded and only accepted rows come back
    (gpe_hm_sample): the same points and the same ``tried``, bit for bit.  ``None``: ``"device"``
    where the set is fused, else ``"host"``."""
    S, mine = _as_set(emuls_or_set)
    try:
        rng = _np.random.default_rng(seed)
        lo = _np.array([S.minmax[k][0] for k in sorted(S.minmax, key=int)], dtype=float)
        hi = _np.array([S.minmax[k][1] for k in sorted(S.minmax, key=int)], dtype=float)
        maxno, count, batch = int(maxno), int(count), int(batch)
        on_device = getattr(S, "fused", False) and getattr(S, "_set", None) is not None
        if generator is None:
            generator = "device" if on_device else "host"
        if generator not in ("host", "device"):
            raise ValueError("generator is 'host', 'device' or None")
        if generator == "device" and not on_device:
            raise RuntimeError("generator='device' needs a fused EmulatorSet")
        kept, have, tried = [], 0, 0
        if generator == "device":
            st = rng.bit_generator.state["state"]
            while have < count and (max_tried is None or tried < max_tried):
                k = batch if max_tried is None else min(batch, int(max_tried) - tried)
                pts, idx, accepted = S._set.sample(lo, hi, st["state"], st["inc"], tried, k, zs, var_extra, cm,
                                                   maxno=maxno, cap=count - have)
                kept.append(pts)
                if have + accepted >= count:
                    return _np.concatenate(kept), int(idx[-1]) + 1
                have += accepted
                tried += k
            return (_np.concatenate(kept) if kept else _np.zeros((0, S.D))), tried
        while have < count and (max_tried is None or tried < max_tried):
            k = batch if max_tried is None else min(batch, int(max_tried) - tried)
            x = lo + rng.random((k, S.D)) * (hi - lo)
            ok = _np.flatnonzero(S.implausibility(zs, var_extra, x, maxno)[:, -maxno] < cm)
            if have + ok.size >= count:
                ok = ok[:count - have]
                kept.append(x[ok])
                return _np.concatenate(kept), tried + int(ok[-1]) + 1
            kept.append(x[ok])
            have += ok.size
            tried += k
        return (_np.concatenate(kept) if kept else _np.zeros((0, S.D))), tried
    finally:
        if mine:
            S.close()
