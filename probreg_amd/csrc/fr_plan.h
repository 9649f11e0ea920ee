// What the deformable kinematic M-step (filterreg_kinematic.hip) sees of a FilterReg plan (filterreg.hip; its lattice: lattice.hip): the plan's
// buffers by pointer (the plan owns them), and the lattice E-step over a moved source that the caller supplies.
#pragma once
#include "prg_common.h"

namespace prg {

struct FrView {
    int device;
    hipStream_t stream;
    int64_t M, N;
    int D, ch;
    const double* src;     // [M][4] source, plan order
    const double* ts;      // [M][4] moved source of the last E-step, plan order
    const float* vout;     // [M][ch] m0, m1(3), m2 of the last E-step, plan order
    double* state;         // [64] device state (0..8 rot, 9..11 t, 12 sigma2)
    const int* src_order;  // host: plan position -> caller's index; null: the caller's order
    bool have_src, have_tgt, have_estep;
    void** kin;                  // the plan's skinning context slot ...
    void (**kin_free)(void*);    // ... and how the plan releases it
};

// flush_slice: finish the last E-step's deferred slice so that `vout` holds its values
int fr_view(prg_filterreg* h, FrView* v, bool flush_slice);
// prg_fr_estep with `moved` ([M][4], plan order, device) in place of the stored source; the state's rot / t must be the identity
int fr_estep_moved(prg_filterreg* h, const double* moved, double alpha, int* lattice_size, int* with_blur);

}  // namespace prg
