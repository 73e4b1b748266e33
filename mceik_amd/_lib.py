"""ctypes binding of libmceik_hip.so (the C-ABI in include/*.h).

The HIP library IS the product: there is no CPU fallback.  If the library is
missing or cannot be loaded this module raises, loudly.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmceik_hip.so")

_lib = None


class FsmBatch(C.Structure):
    """mceik_fsm_batch (include/mceik_eikonal.h)."""
    _fields_ = [("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int),
                ("h", C.c_double), ("x0", C.c_double), ("y0", C.c_double), ("z0", C.c_double),
                ("maxit", C.c_int), ("tol", C.c_double), ("precision", C.c_int),
                ("nmodel", C.c_int), ("nstat", C.c_int), ("nsrc", C.c_int),
                ("src", C.c_void_p), ("slow_mode", C.c_int), ("slow", C.c_void_p),
                ("nrx", C.c_int), ("nry", C.c_int), ("nrz", C.c_int),
                ("nev", C.c_int), ("ev_node", C.c_void_p), ("ttab", C.c_void_p),
                ("u_out", C.c_void_p), ("niter", C.c_void_p), ("ierr", C.c_void_p),
                ("max_sweeps", C.c_int), ("iter_total", C.c_void_p), ("fast_sqrt", C.c_int),
                ("visit_stats", C.c_void_p), ("solve_order", C.c_void_p), ("solve_clock", C.c_void_p),
                ("max_waves", C.c_int), ("traffic", C.c_void_p), ("step_z", C.c_int),
                ("ev_frac", C.c_void_p), ("model_phase", C.c_void_p), ("nphase", C.c_int),
                ("skip", C.c_void_p), ("solve_count", C.c_void_p), ("ev_stride", C.c_int)]


class FsmAdjoint(C.Structure):
    """mceik_fsm_adjoint (include/mceik.h)."""
    _fields_ = [("batch", C.POINTER(FsmBatch)), ("u", C.c_void_p), ("ev_w", C.c_void_p),
                ("grad", C.c_void_p), ("grad_solve", C.c_void_p), ("lam", C.c_void_p),
                ("niter", C.c_void_p), ("status", C.c_void_p), ("maxit", C.c_int), ("max_groups", C.c_int)]


class RelocateBatch(C.Structure):
    """mceik_relocate_batch (include/mceik_eikonal.h)."""
    _fields_ = [("ldgrd", C.c_int), ("ngrd", C.c_int), ("nev", C.c_int), ("iwantOT", C.c_int),
                ("t0use", C.c_float), ("tables", C.c_void_p), ("ev_ptr", C.c_void_p), ("obs_row", C.c_void_p),
                ("tc", C.c_void_p), ("wt", C.c_void_p), ("xnorm", C.c_void_p), ("t0", C.c_void_p),
                ("out", C.c_void_p), ("log_pdf", C.c_int), ("nrows", C.c_int), ("nobs", C.c_int)]


class McmcParms(C.Structure):
    _fields_ = [("resdir", C.c_char * 512), ("nburnIn", C.c_int), ("niter", C.c_int), ("keepK", C.c_int)]


class EikParms(C.Structure):
    _fields_ = [("tol", C.c_double), ("maxit", C.c_int)]


class MceikParms(C.Structure):
    """struct mceik_parms_struct (include/mceik_struct.h; reference mceik_struct.h:68-90)."""
    _fields_ = [("mcparms", McmcParms), ("eikparms", EikParms), ("projnm", C.c_char * 128),
                ("scratch_dir", C.c_char * 512),
                ("x0", C.c_double), ("y0", C.c_double), ("z0", C.c_double),
                ("dx", C.c_double), ("dy", C.c_double), ("dz", C.c_double),
                ("ndivx", C.c_int), ("ndivy", C.c_int), ("ndivz", C.c_int),
                ("nrefx", C.c_int), ("nrefy", C.c_int), ("nrefz", C.c_int)]


class CatalogStruct(C.Structure):
    """struct mceik_catalog_struct (reference mceik_struct.h:10-32)."""
    _fields_ = [(n, C.POINTER(C.c_double)) for n in ("xsrc", "ysrc", "zsrc", "tori", "tobs", "test", "varObs")] + \
               [(n, C.POINTER(C.c_int)) for n in ("luseObs", "pickType", "statPtr", "obsPtr")] + \
               [("nevents", C.c_int)]


class StationsStruct(C.Structure):
    """struct mceik_stations_struct (reference mceik_struct.h:34-49)."""
    _fields_ = [(n, C.POINTER(C.c_char_p)) for n in ("netw", "stnm", "chan", "loc")] + \
               [(n, C.POINTER(C.c_double)) for n in ("xrec", "yrec", "zrec", "pcorr", "scorr")] + \
               [(n, C.POINTER(C.c_int)) for n in ("lhasP", "lhasS")] + \
               [("nstat", C.c_int), ("lcartesian", C.c_int)]


class McmcOpts(C.Structure):
    """mceik_mcmc_opts (include/mceik.h)."""
    _fields_ = [("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int), ("nchains", C.c_int),
                ("chain_offset", C.c_int), ("vmin", C.c_int), ("vmax", C.c_int), ("dvmax", C.c_int),
                ("seed", C.c_uint32), ("max_samples", C.c_int), ("device", C.c_int),
                ("precision", C.c_int), ("max_waves", C.c_int), ("tt_interp", C.c_int),
                ("nphase", C.c_int), ("vsmin", C.c_int), ("vsmax", C.c_int), ("mask_s", C.c_int)]


class McmcInfo(C.Structure):
    """mceik_mcmc_info (include/mceik.h)."""
    _fields_ = [("npipe", C.c_int), ("nphase", C.c_int), ("step_z", C.c_int), ("fixed_layout", C.c_int),
                ("chains", C.c_int * 4), ("waves", C.c_int * 4), ("workspace_bytes", C.c_size_t * 4),
                ("lds_bytes", C.c_size_t), ("masked_s", C.c_int), ("kernel", C.c_char * 64),
                ("multi_step", C.c_int)]


class PosteriorOpts(C.Structure):
    """mceik_posterior_opts (include/mceik.h)."""
    _fields_ = [("per_chain", C.c_int), ("nbins", C.c_int)]


class PosteriorPartials(C.Structure):
    """mceik_posterior_partials (include/mceik.h): caller-allocated host arrays."""
    _fields_ = [("ncm", C.c_int), ("nbins", C.c_int), ("per_chain", C.c_int),
                ("nchains", C.c_longlong), ("nkept", C.c_longlong),
                ("S", C.c_void_p), ("Q", C.c_void_p), ("P", C.c_void_p), ("hist", C.c_void_p)]


class TemperOpts(C.Structure):
    """mceik_temper_opts (include/mceik.h)."""
    _fields_ = [("ntemps", C.c_int), ("swap_every", C.c_int), ("beta", C.c_void_p)]


class BlockOpts(C.Structure):
    """mceik_block_opts (include/mceik.h)."""
    _fields_ = [("rmin", C.c_int), ("rmax", C.c_int)]


class PriorOpts(C.Structure):
    """mceik_prior_opts (include/mceik.h)."""
    _fields_ = [("w_smooth", C.c_double * 2), ("w_damp", C.c_double * 2), ("vref", C.c_void_p)]


class HypoOpts(C.Structure):
    """mceik_hypo_opts (include/mceik.h)."""
    _fields_ = [("every", C.c_int), ("dmax", C.c_int * 3), ("lo", C.c_int * 3), ("hi", C.c_int * 3)]


class NuisOpts(C.Structure):
    """mceik_nuis_opts (include/mceik.h)."""
    _fields_ = [("every", C.c_int), ("offset", C.c_int), ("nsub", C.c_int), ("noise", C.c_int), ("statics", C.c_int),
                ("nk", C.c_int), ("dk", C.c_int), ("dc", C.c_int), ("kcmax", C.c_int), ("dt", C.c_double),
                ("lam", C.c_void_p), ("lnlam", C.c_void_p), ("norm", C.c_void_p)]


class VorOpts(C.Structure):
    """mceik_vor_opts (include/mceik.h)."""
    _fields_ = [("kmin", C.c_int), ("kmax", C.c_int), ("k0", C.c_int), ("dv", C.c_int), ("dmax", C.c_int * 3),
                ("metric", C.c_int * 3)]


class DeOpts(C.Structure):
    """mceik_de_opts (include/mceik.h)."""
    _fields_ = [("every", C.c_int), ("offset", C.c_int), ("gamma_q16", C.c_int), ("cr_q16", C.c_int)]


class LangOpts(C.Structure):
    """mceik_lang_opts (include/mceik.h)."""
    _fields_ = [("every", C.c_int), ("offset", C.c_int), ("sigma", C.c_double), ("dmax", C.c_int),
                ("mem_bytes", C.c_size_t)]


LANG_DMAX_CAP = 32
COV_MAX_PROBES = 64


class CovOpts(C.Structure):
    """mceik_cov_opts (include/mceik.h)."""
    _fields_ = [("np", C.c_int), ("kind", C.c_int * COV_MAX_PROBES), ("index", C.c_int * COV_MAX_PROBES),
                ("within", C.c_int)]


class CovPartials(C.Structure):
    """mceik_cov_partials (include/mceik.h): caller-allocated host arrays."""
    _fields_ = [("np", C.c_int), ("ncm", C.c_int), ("within", C.c_int),
                ("kind", C.c_int * COV_MAX_PROBES), ("index", C.c_int * COV_MAX_PROBES),
                ("nchains", C.c_longlong), ("nkept", C.c_longlong),
                ("A", C.c_void_p), ("S", C.c_void_p), ("G", C.c_void_p), ("Q", C.c_void_p), ("C", C.c_void_p),
                ("PA", C.c_void_p), ("P", C.c_void_p), ("T", C.c_void_p)]


ESS_MAX_LEVELS = 16


class EssOpts(C.Structure):
    """mceik_ess_opts (include/mceik.h)."""
    _fields_ = [("nlevels", C.c_int), ("np", C.c_int), ("kind", C.c_int * COV_MAX_PROBES),
                ("index", C.c_int * COV_MAX_PROBES)]


class EssPartials(C.Structure):
    """mceik_ess_partials (include/mceik.h): caller-allocated host arrays."""
    _fields_ = [("ncm", C.c_int), ("np", C.c_int), ("nlevels", C.c_int),
                ("nchains", C.c_longlong), ("nkept", C.c_longlong),
                ("A", C.c_void_p), ("Q", C.c_void_p), ("P", C.c_void_p)]


FIT_MAX_BINS = 256


class FitOpts(C.Structure):
    """mceik_fit_opts (include/mceik.h)."""
    _fields_ = [("tick", C.c_double), ("nbins", C.c_int), ("zmax", C.c_double), ("t0_ref", C.c_void_p)]


class FitPartials(C.Structure):
    """mceik_fit_partials (include/mceik.h): caller-allocated host arrays."""
    _fields_ = [("nobs", C.c_int), ("nev", C.c_int), ("nphase", C.c_int), ("nstat", C.c_int), ("nbins", C.c_int),
                ("tick", C.c_double), ("zmax", C.c_double),
                ("nchains", C.c_longlong), ("nkept", C.c_longlong),
                ("obs_ptr", C.c_void_p), ("obs_stat", C.c_void_p), ("obs_phase", C.c_void_p), ("obs_mask", C.c_void_p),
                ("t0_ref", C.c_void_p),
                ("sq", C.c_void_p), ("szq", C.c_void_p), ("sq2", C.c_void_p), ("szq2", C.c_void_p),
                ("stq", C.c_void_p), ("stq2", C.c_void_p), ("hist", C.c_void_p),
                ("sat", C.c_longlong * 3)]


# every extern "C" symbol include/*.h declares
EXPORTS = ("eikonal3d_serial_driver", "eikonal3d_serial_driver_sp", "eikonal3d_batch_solve", "eikonal3d_initialize", "eikonal3d_solve",
           "eikonal3d_finalize", "locate3d_gridsearch__double64", "locate3d_gridsearch__float64",
           "locate_l2_gridSearch__double64",
           "locate_l2_gridSearch__float64", "mceik_relocate",
           "locate_l1_gridSearch__double64", "mceik_relocate_l1", "weightedMedian__double",
           "mceik_mcmc_likelihood_set", "mceik_mcmc_likelihood_get", "mceik_l1_event",
           "locate3d_initialize", "locate3d_gridsearch", "locate3d_finalize",
           "mceik_fsm_workspace_bytes", "mceik_fsm_batch_solve", "mceik_fsm_bytes_per_node_sweep", "mceik_fsm_step_z",
           "mceik_fsm_kernel_name", "mceik_fsm_lds_bytes", "mceik_fsm_check",
           "mceik_fsm_adjoint_workspace_bytes", "mceik_fsm_adjoint_check", "mceik_fsm_adjoint_solve",
           "mceik_memcpy",
           "mceik_mcmc_init", "mceik_mcmc_run", "mceik_mcmc_set_stream", "mceik_mcmc_sync",
           "mceik_mcmc_get_state", "mceik_mcmc_get_samples", "mceik_mcmc_last", "mceik_mcmc_fsm_stats",
           "mceik_mcmc_checkpoint", "mceik_mcmc_restore", "mceik_mcmc_finalize", "mceik_mcmc_last_phase",
           "mceik_mcmc_get_info", "mceik_mcmc_fsm_solves",
           "mceik_mcmc_posterior_enable", "mceik_mcmc_posterior_disable", "mceik_mcmc_posterior_accumulate",
           "mceik_mcmc_posterior_get", "mceik_mcmc_posterior_set", "mceik_mcmc_posterior_partials",
           "mceik_posterior_merge", "mceik_posterior_finish",
           "mceik_mcmc_temper_enable", "mceik_mcmc_temper_disable", "mceik_mcmc_temper_get",
           "mceik_mcmc_temper_stats", "mceik_mcmc_temper_swap", "mceik_temper_ladder",
           "mceik_mcmc_block_enable", "mceik_mcmc_block_disable", "mceik_mcmc_block_get", "mceik_mcmc_block_stats",
           "mceik_block_footprint",
           "mceik_mcmc_prior_enable", "mceik_mcmc_prior_disable", "mceik_mcmc_prior_get", "mceik_mcmc_prior_energy",
           "mceik_mcmc_prior_last", "mceik_prior_energy", "mceik_prior_delta",
           "mceik_mcmc_hypo_enable", "mceik_mcmc_hypo_disable", "mceik_mcmc_hypo_get", "mceik_mcmc_hypo_set",
           "mceik_mcmc_hypo_stats", "mceik_mcmc_hypo_last", "mceik_mcmc_hypo_moments_get",
           "mceik_mcmc_hypo_moments_set", "mceik_hypo_draw",
           "mceik_mcmc_nuis_enable", "mceik_mcmc_nuis_disable", "mceik_mcmc_nuis_clear", "mceik_mcmc_nuis_get",
           "mceik_mcmc_nuis_set", "mceik_mcmc_nuis_stats", "mceik_mcmc_nuis_last", "mceik_mcmc_nuis_moments_get",
           "mceik_mcmc_nuis_moments_set", "mceik_nuis_draw",
           "mceik_mcmc_cov_enable", "mceik_mcmc_cov_disable", "mceik_mcmc_cov_clear", "mceik_mcmc_cov_accumulate",
           "mceik_mcmc_cov_get", "mceik_mcmc_cov_set", "mceik_mcmc_cov_partials", "mceik_cov_merge", "mceik_cov_finish",
           "mceik_mcmc_ess_enable", "mceik_mcmc_ess_disable", "mceik_mcmc_ess_clear", "mceik_mcmc_ess_accumulate",
           "mceik_mcmc_ess_get", "mceik_mcmc_ess_set", "mceik_mcmc_ess_partials", "mceik_ess_check", "mceik_ess_lstar",
           "mceik_ess_merge", "mceik_ess_finish",
           "mceik_mcmc_fit_enable", "mceik_mcmc_fit_disable", "mceik_mcmc_fit_clear", "mceik_mcmc_fit_accumulate",
           "mceik_mcmc_fit_get", "mceik_mcmc_fit_set", "mceik_mcmc_fit_partials", "mceik_mcmc_fit_last",
           "mceik_fit_check", "mceik_fit_merge", "mceik_fit_finish",
           "mceik_mcmc_lang_enable", "mceik_mcmc_lang_disable", "mceik_mcmc_lang_get", "mceik_mcmc_lang_stats",
           "mceik_mcmc_lang_last", "mceik_det_exp", "mceik_lang_cell",
           "mceik_mcmc_de_enable", "mceik_mcmc_de_disable", "mceik_mcmc_de_get", "mceik_mcmc_de_stats",
           "mceik_mcmc_de_last", "mceik_de_delta", "mceik_de_draw",
           "mceik_mcmc_vor_enable", "mceik_mcmc_vor_disable", "mceik_mcmc_vor_get", "mceik_mcmc_vor_set",
           "mceik_mcmc_vor_rasterize", "mceik_mcmc_vor_stats", "mceik_mcmc_vor_last", "mceik_mcmc_vor_moments", "mceik_mcmc_vor_moments_set",
           "mceik_vor_raster", "mceik_vor_free_cell", "mceik_vor_draw",
           "mceik_parms_defaults", "mceik_parms_set", "mceik_parms_read", "mceik_parms_args", "mceik_parms_write",
           "mceik_comm_available", "mceik_comm_unique_id", "mceik_comm_init", "mceik_comm_finalize", "mceik_mcmc_gather",
           "os_path_exists", "os_path_isdir", "os_path_isfile", "os_makedirs", "os_mkdir")


def lib():
    """Load libmceik_hip.so (raises OSError/ImportError if absent: no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"mceik_amd: HIP library {LIB_PATH} is missing; build it with "
                          f"`make -C {_HERE}` (or __graft_entry__.build()). No CPU fallback exists.")
    L = C.CDLL(LIB_PATH)
    pi = C.POINTER(C.c_int); pd = C.POINTER(C.c_double)
    for name in ("eikonal3d_serial_driver", "eikonal3d_serial_driver_sp"):
        f = getattr(L, name)
        f.restype = None
        f.argtypes = [pi] * 7 + [pd] * 5 + [C.c_void_p] * 6 + [pi]
    L.eikonal3d_initialize.restype = None
    L.eikonal3d_initialize.argtypes = [pi] * 10 + [pd] * 5 + [pi]
    L.eikonal3d_solve.restype = None
    L.eikonal3d_solve.argtypes = [pi] * 3 + [C.c_void_p] * 6 + [pi]
    L.eikonal3d_finalize.restype = None
    L.eikonal3d_finalize.argtypes = [pi, pi]
    for name in ("locate3d_gridsearch__double64", "locate3d_gridsearch__float64"):
        f = getattr(L, name)
        f.restype = None
        f.argtypes = [pi] * 4 + [C.c_void_p] * 5 + [pi]
    L.locate_l2_gridSearch__double64.restype = C.c_int
    L.locate_l2_gridSearch__double64.argtypes = [C.c_int] * 4 + [C.c_double] + [C.c_void_p] * 7
    L.eikonal3d_batch_solve.restype = C.c_int
    L.eikonal3d_batch_solve.argtypes = [C.c_int] * 5 + [C.c_double] * 4 + [C.c_int, C.c_double] + [C.c_void_p] * 5
    L.mceik_fsm_workspace_bytes.restype = C.c_size_t
    L.mceik_fsm_workspace_bytes.argtypes = [C.POINTER(FsmBatch)]
    L.mceik_fsm_step_z.restype = C.c_int
    L.mceik_fsm_step_z.argtypes = [C.POINTER(FsmBatch)]
    L.mceik_fsm_kernel_name.restype = C.c_char_p
    L.mceik_fsm_kernel_name.argtypes = [C.POINTER(FsmBatch)]
    L.mceik_fsm_lds_bytes.restype = C.c_size_t
    L.mceik_fsm_lds_bytes.argtypes = [C.POINTER(FsmBatch)]
    L.mceik_fsm_check.restype = C.c_int
    L.mceik_fsm_check.argtypes = [C.POINTER(FsmBatch)]
    L.mceik_fsm_bytes_per_node_sweep.restype = C.c_double
    L.mceik_fsm_bytes_per_node_sweep.argtypes = [C.POINTER(FsmBatch)]
    L.mceik_fsm_batch_solve.restype = C.c_int
    L.mceik_fsm_batch_solve.argtypes = [C.POINTER(FsmBatch), C.c_void_p, C.c_size_t, C.c_void_p]
    L.mceik_fsm_adjoint_workspace_bytes.restype = C.c_size_t
    L.mceik_fsm_adjoint_workspace_bytes.argtypes = [C.POINTER(FsmAdjoint)]
    L.mceik_fsm_adjoint_check.restype = C.c_int
    L.mceik_fsm_adjoint_check.argtypes = [C.POINTER(FsmAdjoint)]
    L.mceik_fsm_adjoint_solve.restype = C.c_int
    L.mceik_fsm_adjoint_solve.argtypes = [C.POINTER(FsmAdjoint), C.c_void_p, C.c_size_t, C.c_void_p]
    L.mceik_memcpy.restype = C.c_int
    L.mceik_memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L.locate_l2_gridSearch__float64.restype = C.c_int
    L.locate_l2_gridSearch__float64.argtypes = [C.c_int] * 4 + [C.c_float] + [C.c_void_p] * 7
    L.mceik_relocate.restype = C.c_int
    L.mceik_relocate.argtypes = [C.POINTER(RelocateBatch), C.c_void_p]
    L.locate_l1_gridSearch__double64.restype = C.c_int
    L.locate_l1_gridSearch__double64.argtypes = [C.c_int] * 4 + [C.c_double] + [C.c_void_p] * 6
    L.mceik_relocate_l1.restype = C.c_int
    L.mceik_relocate_l1.argtypes = [C.POINTER(RelocateBatch), C.c_void_p]
    L.weightedMedian__double.restype = C.c_double
    L.weightedMedian__double.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_bool), pi]
    L.mceik_l1_event.restype = C.c_int
    L.mceik_l1_event.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, pd, pd]
    L.mceik_mcmc_likelihood_set.restype = C.c_int
    L.mceik_mcmc_likelihood_set.argtypes = [C.c_void_p, C.c_int]
    L.mceik_mcmc_likelihood_get.restype = C.c_int
    L.mceik_mcmc_likelihood_get.argtypes = [C.c_void_p]
    L.mceik_mcmc_init.restype = C.c_int
    L.mceik_mcmc_init.argtypes = [C.POINTER(MceikParms), C.POINTER(StationsStruct), C.POINTER(CatalogStruct),
                                  C.POINTER(McmcOpts), C.c_void_p, C.POINTER(C.c_void_p)]
    L.mceik_mcmc_run.restype = C.c_int
    L.mceik_mcmc_run.argtypes = [C.c_void_p, C.c_int]
    L.mceik_mcmc_set_stream.restype = C.c_int
    L.mceik_mcmc_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    L.mceik_mcmc_sync.restype = C.c_int
    L.mceik_mcmc_sync.argtypes = [C.c_void_p]
    L.mceik_mcmc_get_state.restype = C.c_int
    L.mceik_mcmc_get_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_longlong)]
    L.mceik_mcmc_get_samples.restype = C.c_int
    L.mceik_mcmc_get_samples.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, pi]
    L.mceik_mcmc_last.restype = C.c_int
    L.mceik_mcmc_last.argtypes = [C.c_void_p] + [C.POINTER(C.c_void_p)] * 4
    L.mceik_mcmc_checkpoint.restype = C.c_int
    L.mceik_mcmc_checkpoint.argtypes = [C.c_void_p] + [C.c_void_p] * 3 + [C.POINTER(C.c_longlong), pi]
    L.mceik_mcmc_restore.restype = C.c_int
    L.mceik_mcmc_restore.argtypes = [C.c_void_p] + [C.c_void_p] * 3 + [C.c_longlong, C.c_int]
    L.mceik_mcmc_fsm_stats.restype = C.c_int
    L.mceik_mcmc_fsm_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_longlong),
                                       C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), C.c_int]
    L.mceik_mcmc_fsm_solves.restype = C.c_int
    L.mceik_mcmc_fsm_solves.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
    L.mceik_comm_available.restype = C.c_int
    L.mceik_comm_available.argtypes = []
    L.mceik_comm_unique_id.restype = C.c_int
    L.mceik_comm_unique_id.argtypes = [C.c_void_p]
    L.mceik_comm_init.restype = C.c_int
    L.mceik_comm_init.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.mceik_comm_finalize.restype = C.c_int
    L.mceik_comm_finalize.argtypes = [C.POINTER(C.c_void_p)]
    L.mceik_mcmc_gather.restype = C.c_int
    L.mceik_mcmc_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.mceik_mcmc_last_phase.restype = C.c_int
    L.mceik_mcmc_last_phase.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.mceik_mcmc_get_info.restype = C.c_int
    L.mceik_mcmc_get_info.argtypes = [C.c_void_p, C.POINTER(McmcInfo)]
    L.mceik_mcmc_finalize.restype = C.c_int
    L.mceik_mcmc_finalize.argtypes = [C.POINTER(C.c_void_p)]
    L.mceik_mcmc_posterior_enable.restype = C.c_int
    L.mceik_mcmc_posterior_enable.argtypes = [C.c_void_p, C.POINTER(PosteriorOpts)]
    L.mceik_mcmc_posterior_disable.restype = C.c_int
    L.mceik_mcmc_posterior_disable.argtypes = [C.c_void_p]
    L.mceik_mcmc_posterior_accumulate.restype = C.c_int
    L.mceik_mcmc_posterior_accumulate.argtypes = [C.c_void_p]
    L.mceik_mcmc_posterior_get.restype = C.c_int
    L.mceik_mcmc_posterior_get.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)] + [C.c_void_p] * 3
    L.mceik_mcmc_posterior_set.restype = C.c_int
    L.mceik_mcmc_posterior_set.argtypes = [C.c_void_p, C.c_longlong] + [C.c_void_p] * 3
    L.mceik_mcmc_posterior_partials.restype = C.c_int
    L.mceik_mcmc_posterior_partials.argtypes = [C.c_void_p, C.POINTER(PosteriorPartials)]
    L.mceik_posterior_merge.restype = C.c_int
    L.mceik_posterior_merge.argtypes = [C.POINTER(PosteriorPartials), C.POINTER(PosteriorPartials)]
    L.mceik_posterior_finish.restype = C.c_int
    L.mceik_posterior_finish.argtypes = [C.POINTER(PosteriorPartials)] + [C.c_void_p] * 3
    L.mceik_mcmc_temper_enable.restype = C.c_int
    L.mceik_mcmc_temper_enable.argtypes = [C.c_void_p, C.POINTER(TemperOpts)]
    L.mceik_mcmc_temper_disable.restype = C.c_int
    L.mceik_mcmc_temper_disable.argtypes = [C.c_void_p]
    L.mceik_mcmc_temper_get.restype = C.c_int
    L.mceik_mcmc_temper_get.argtypes = [C.c_void_p, pi, pi, C.c_void_p]
    L.mceik_mcmc_temper_stats.restype = C.c_int
    L.mceik_mcmc_temper_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.mceik_mcmc_temper_swap.restype = C.c_int
    L.mceik_mcmc_temper_swap.argtypes = [C.c_void_p, C.c_int]
    L.mceik_temper_ladder.restype = C.c_int
    L.mceik_temper_ladder.argtypes = [C.c_int, C.c_double, C.c_void_p]
    L.mceik_mcmc_block_enable.restype = C.c_int
    L.mceik_mcmc_block_enable.argtypes = [C.c_void_p, C.POINTER(BlockOpts)]
    L.mceik_mcmc_block_disable.restype = C.c_int
    L.mceik_mcmc_block_disable.argtypes = [C.c_void_p]
    L.mceik_mcmc_block_get.restype = C.c_int
    L.mceik_mcmc_block_get.argtypes = [C.c_void_p, pi, pi]
    L.mceik_mcmc_block_stats.restype = C.c_int
    L.mceik_mcmc_block_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.mceik_block_footprint.restype = C.c_int
    L.mceik_block_footprint.argtypes = [C.c_int] * 6 + [C.c_void_p, C.c_void_p]
    L.mceik_mcmc_lang_enable.restype = C.c_int
    L.mceik_mcmc_lang_enable.argtypes = [C.c_void_p, C.POINTER(LangOpts)]
    L.mceik_mcmc_lang_disable.restype = C.c_int
    L.mceik_mcmc_lang_disable.argtypes = [C.c_void_p]
    L.mceik_mcmc_lang_get.restype = C.c_int
    L.mceik_mcmc_lang_get.argtypes = [C.c_void_p, C.POINTER(LangOpts), C.c_void_p]
    L.mceik_mcmc_lang_stats.restype = C.c_int
    L.mceik_mcmc_lang_stats.argtypes = [C.c_void_p] + [C.POINTER(C.c_longlong)] * 4 + [C.c_int]
    L.mceik_mcmc_lang_last.restype = C.c_int
    L.mceik_mcmc_lang_last.argtypes = [C.c_void_p] * 8
    L.mceik_det_exp.restype = C.c_double
    L.mceik_det_exp.argtypes = [C.c_double]
    L.mceik_lang_cell.restype = C.c_int
    L.mceik_lang_cell.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int,
                                  C.c_double, C.c_int, pi, pi, pi, C.c_void_p]
    L.mceik_mcmc_de_enable.restype = C.c_int
    L.mceik_mcmc_de_enable.argtypes = [C.c_void_p, C.POINTER(DeOpts)]
    L.mceik_mcmc_de_disable.restype = C.c_int
    L.mceik_mcmc_de_disable.argtypes = [C.c_void_p]
    L.mceik_mcmc_de_get.restype = C.c_int
    L.mceik_mcmc_de_get.argtypes = [C.c_void_p, C.POINTER(DeOpts)]
    L.mceik_mcmc_de_stats.restype = C.c_int
    L.mceik_mcmc_de_stats.argtypes = [C.c_void_p] + [C.POINTER(C.c_longlong)] * 5 + [C.c_int]
    L.mceik_mcmc_de_last.restype = C.c_int
    L.mceik_mcmc_de_last.argtypes = [C.c_void_p] * 10
    L.mceik_de_delta.restype = C.c_int
    L.mceik_de_delta.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_int, pi]
    L.mceik_de_draw.restype = C.c_int
    L.mceik_de_draw.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_int, pi, pi, C.POINTER(C.c_double)]
    L.mceik_mcmc_vor_enable.restype = C.c_int
    L.mceik_mcmc_vor_enable.argtypes = [C.c_void_p, C.POINTER(VorOpts), C.c_void_p, C.c_void_p, C.c_void_p]
    L.mceik_mcmc_vor_disable.restype = C.c_int
    L.mceik_mcmc_vor_disable.argtypes = [C.c_void_p]
    L.mceik_mcmc_vor_get.restype = C.c_int
    L.mceik_mcmc_vor_get.argtypes = [C.c_void_p, C.POINTER(VorOpts), pi, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mceik_mcmc_vor_set.restype = C.c_int
    L.mceik_mcmc_vor_set.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.mceik_mcmc_vor_rasterize.restype = C.c_int
    L.mceik_mcmc_vor_rasterize.argtypes = [C.c_void_p]
    L.mceik_mcmc_vor_stats.restype = C.c_int
    L.mceik_mcmc_vor_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.mceik_mcmc_vor_last.restype = C.c_int
    L.mceik_mcmc_vor_last.argtypes = [C.c_void_p] * 9
    L.mceik_mcmc_vor_moments.restype = C.c_int
    L.mceik_mcmc_vor_moments.argtypes = [C.c_void_p, C.POINTER(C.c_longlong), C.c_void_p, C.c_void_p]
    L.mceik_mcmc_vor_moments_set.restype = C.c_int
    L.mceik_mcmc_vor_moments_set.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]
    L.mceik_vor_raster.restype = C.c_int
    L.mceik_vor_raster.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.mceik_vor_free_cell.restype = C.c_int
    L.mceik_vor_free_cell.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.mceik_vor_draw.restype = C.c_int
    L.mceik_vor_draw.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
    L.mceik_mcmc_prior_enable.restype = C.c_int
    L.mceik_mcmc_prior_enable.argtypes = [C.c_void_p, C.POINTER(PriorOpts)]
    L.mceik_mcmc_prior_disable.restype = C.c_int
    L.mceik_mcmc_prior_disable.argtypes = [C.c_void_p]
    L.mceik_mcmc_prior_get.restype = C.c_int
    L.mceik_mcmc_prior_get.argtypes = [C.c_void_p, C.POINTER(PriorOpts), C.c_void_p]
    L.mceik_mcmc_prior_energy.restype = C.c_int
    L.mceik_mcmc_prior_energy.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.mceik_mcmc_prior_last.restype = C.c_int
    L.mceik_mcmc_prior_last.argtypes = [C.c_void_p, C.c_void_p]
    L.mceik_prior_energy.restype = C.c_int
    L.mceik_prior_energy.argtypes = [C.c_int] * 3 + [C.c_void_p] * 2 + [C.POINTER(C.c_longlong)] * 2
    L.mceik_prior_delta.restype = C.c_int
    L.mceik_prior_delta.argtypes = [C.c_int] * 3 + [C.c_void_p] * 2 + [C.c_int] * 3 + [C.POINTER(C.c_longlong)] * 2
    L.mceik_mcmc_hypo_enable.restype = C.c_int
    L.mceik_mcmc_hypo_enable.argtypes = [C.c_void_p, C.POINTER(HypoOpts)]
    L.mceik_mcmc_hypo_disable.restype = C.c_int
    L.mceik_mcmc_hypo_disable.argtypes = [C.c_void_p]
    L.mceik_mcmc_hypo_get.restype = C.c_int
    L.mceik_mcmc_hypo_get.argtypes = [C.c_void_p, C.POINTER(HypoOpts), C.c_void_p]
    L.mceik_mcmc_hypo_set.restype = C.c_int
    L.mceik_mcmc_hypo_set.argtypes = [C.c_void_p, C.c_void_p]
    L.mceik_mcmc_hypo_stats.restype = C.c_int
    L.mceik_mcmc_hypo_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.mceik_mcmc_hypo_last.restype = C.c_int
    L.mceik_mcmc_hypo_last.argtypes = [C.c_void_p] * 4
    L.mceik_mcmc_hypo_moments_get.restype = C.c_int
    L.mceik_mcmc_hypo_moments_get.argtypes = [C.c_void_p, C.POINTER(C.c_longlong), C.c_void_p, C.c_void_p]
    L.mceik_mcmc_hypo_moments_set.restype = C.c_int
    L.mceik_mcmc_hypo_moments_set.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]
    L.mceik_hypo_draw.restype = C.c_int
    L.mceik_hypo_draw.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p,
                                  C.POINTER(C.c_double)]
    L.mceik_mcmc_nuis_enable.restype = C.c_int
    L.mceik_mcmc_nuis_enable.argtypes = [C.c_void_p, C.POINTER(NuisOpts)]
    for name in ("mceik_mcmc_nuis_disable", "mceik_mcmc_nuis_clear"):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = [C.c_void_p]
    L.mceik_mcmc_nuis_get.restype = C.c_int
    L.mceik_mcmc_nuis_get.argtypes = [C.c_void_p, C.POINTER(NuisOpts)] + [C.c_void_p] * 5
    L.mceik_mcmc_nuis_set.restype = C.c_int
    L.mceik_mcmc_nuis_set.argtypes = [C.c_void_p] * 3
    L.mceik_mcmc_nuis_stats.restype = C.c_int
    L.mceik_mcmc_nuis_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.mceik_mcmc_nuis_last.restype = C.c_int
    L.mceik_mcmc_nuis_last.argtypes = [C.c_void_p] * 3
    L.mceik_mcmc_nuis_moments_get.restype = C.c_int
    L.mceik_mcmc_nuis_moments_get.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)] + [C.c_void_p] * 3
    L.mceik_mcmc_nuis_moments_set.restype = C.c_int
    L.mceik_mcmc_nuis_moments_set.argtypes = [C.c_void_p, C.c_longlong] + [C.c_void_p] * 3
    L.mceik_nuis_draw.restype = C.c_int
    L.mceik_nuis_draw.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64] + [C.c_int] * 6 + [C.c_void_p, C.POINTER(C.c_double)]
    L.mceik_mcmc_cov_enable.restype = C.c_int
    L.mceik_mcmc_cov_enable.argtypes = [C.c_void_p, C.POINTER(CovOpts)]
    for name in ("mceik_mcmc_cov_disable", "mceik_mcmc_cov_clear", "mceik_mcmc_cov_accumulate"):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = [C.c_void_p]
    L.mceik_mcmc_cov_get.restype = C.c_int
    L.mceik_mcmc_cov_get.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)] + [C.c_void_p] * 7
    L.mceik_mcmc_cov_set.restype = C.c_int
    L.mceik_mcmc_cov_set.argtypes = [C.c_void_p, C.c_longlong] + [C.c_void_p] * 7
    L.mceik_mcmc_cov_partials.restype = C.c_int
    L.mceik_mcmc_cov_partials.argtypes = [C.c_void_p, C.POINTER(CovPartials)]
    L.mceik_cov_merge.restype = C.c_int
    L.mceik_cov_merge.argtypes = [C.POINTER(CovPartials), C.POINTER(CovPartials)]
    L.mceik_cov_finish.restype = C.c_int
    L.mceik_cov_finish.argtypes = [C.POINTER(CovPartials)] + [C.c_void_p] * 9
    L.mceik_mcmc_ess_enable.restype = C.c_int
    L.mceik_mcmc_ess_enable.argtypes = [C.c_void_p, C.POINTER(EssOpts)]
    for name in ("mceik_mcmc_ess_disable", "mceik_mcmc_ess_clear", "mceik_mcmc_ess_accumulate"):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = [C.c_void_p]
    L.mceik_mcmc_ess_get.restype = C.c_int
    L.mceik_mcmc_ess_get.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)] + [C.c_void_p] * 5
    L.mceik_mcmc_ess_set.restype = C.c_int
    L.mceik_mcmc_ess_set.argtypes = [C.c_void_p, C.c_longlong] + [C.c_void_p] * 5
    L.mceik_mcmc_ess_partials.restype = C.c_int
    L.mceik_mcmc_ess_partials.argtypes = [C.c_void_p, C.POINTER(EssPartials)]
    L.mceik_ess_check.restype = C.c_int
    L.mceik_ess_check.argtypes = [C.c_int, C.c_longlong]
    L.mceik_ess_lstar.restype = C.c_int
    L.mceik_ess_lstar.argtypes = [C.c_int, C.c_longlong]
    L.mceik_ess_merge.restype = C.c_int
    L.mceik_ess_merge.argtypes = [C.POINTER(EssPartials), C.POINTER(EssPartials)]
    L.mceik_ess_finish.restype = C.c_int
    L.mceik_ess_finish.argtypes = [C.POINTER(EssPartials), C.c_int] + [C.c_void_p] * 3 + [pi]
    L.mceik_mcmc_fit_enable.restype = C.c_int
    L.mceik_mcmc_fit_enable.argtypes = [C.c_void_p, C.POINTER(FitOpts)]
    for name in ("mceik_mcmc_fit_disable", "mceik_mcmc_fit_clear", "mceik_mcmc_fit_accumulate"):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = [C.c_void_p]
    L.mceik_mcmc_fit_get.restype = C.c_int
    L.mceik_mcmc_fit_get.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)] + [C.c_void_p] * 8
    L.mceik_mcmc_fit_set.restype = C.c_int
    L.mceik_mcmc_fit_set.argtypes = [C.c_void_p, C.c_longlong] + [C.c_void_p] * 8
    L.mceik_mcmc_fit_partials.restype = C.c_int
    L.mceik_mcmc_fit_partials.argtypes = [C.c_void_p, C.POINTER(FitPartials)]
    L.mceik_mcmc_fit_last.restype = C.c_int
    L.mceik_mcmc_fit_last.argtypes = [C.c_void_p] * 4
    L.mceik_fit_check.restype = C.c_int
    L.mceik_fit_check.argtypes = [C.c_double, C.c_double]
    L.mceik_fit_merge.restype = C.c_int
    L.mceik_fit_merge.argtypes = [C.POINTER(FitPartials), C.POINTER(FitPartials)]
    L.mceik_fit_finish.restype = C.c_int
    L.mceik_fit_finish.argtypes = [C.POINTER(FitPartials)] + [C.c_void_p] * 10
    _lib = L
    return L
