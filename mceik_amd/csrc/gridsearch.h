// gridsearch.h -- host launchers of the location grid-search kernels
// (mcmc_kernels.hip), C++ linkage; locate_dropin.hip is their caller.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

hipError_t gridsearch_f90(int is_double, int ldgrd, int ngrd, int nuse, int iwantOT, const int *row,
                          const void *tob, const void *w0, const void *wl, const void *test, void *logpdf,
                          hipStream_t st);
hipError_t l2_gridsearch(int ldgrd, int ngrd, int nuse, int iwantOT, double t0use, const int *use,
                         const double *tc, const double *wt, double xnorm, const double *test,
                         double *t0, double *objfn, hipStream_t st);
hipError_t l2_gridsearch_f32(int ldgrd, int ngrd, int nev, int iwantOT, float t0use, const int *ev_ptr,
                             const int *obs_row, const float *tc, const float *wt, const float *xnorm,
                             const float *test, float *t0, float *objfn, int negate, hipStream_t st);
size_t relocate_lds_bytes(int nrows, int nobs, int nev);
hipError_t relocate_lds(int ldgrd, int ngrd, int nrows, int nev, int nobs, int iwantOT, float t0use,
                        const int *ev_ptr, const int *obs_row, const float *tc, const float *wt, const float *xnorm,
                        const float *test, float *t0, float *objfn, int negate, hipStream_t st);
