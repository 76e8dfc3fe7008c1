// step.hip -- one exact-GP training step of the plain MOSM kernel behind ONE call: raw parameters -> term table (hoststep.hip) ->
// mogp_model_set_terms -> the gradient evaluation (mogp_exact_eval, unchanged: same launches in the same order) -> raw gradient (hoststep.hip).
// Reference: gpr/model.py:279-292 (Model.loss: forward, backward).  Between the moment kernel of one step and the first chain kernel of the
// next the device waits for exactly this host section, so it is native code end to end; nothing of it runs on the device.
#include "mogp_model.h"

using namespace mogp;

extern "C" {

int mogp_exact_step(mogp_model* m, int C, int Q, int D, int nscale, const double* raw, const int* tkind, const double* lower, const double* upper,
                    const double* beta, const double* threshold, const double* lp, const double* en, double twopi, double phase_scale,
                    const double* data_var, double jitter,
                    const double* counts, const int* trained, double* cons, double* dcons, double* table, double* noise_var, double* moments,
                    double* diagG, double* out5, double* graw, int64_t* info) {
    if (!m || !out5) return fail(MOGP_EINVAL, "mogp_exact_step: null argument");
    if (C != m->C || D != m->D) return fail(MOGP_EINVAL, "mogp_exact_step: C and D must be the model's");
    int rc;
    if ((rc = mogp_mosm_step_forward(C, Q, D, nscale, raw, tkind, lower, upper, beta, threshold, lp, en, twopi, phase_scale, cons, dcons, table, noise_var)))
        return fail(rc, "mogp_exact_step: bad argument (forward)");
    if ((rc = mogp_model_set_terms(m, Q, table))) return rc;
    double lml = 0.0, trG = 0.0, jit = 0.0;
    if ((rc = mogp_exact_eval(m, noise_var, data_var, jitter, MOGP_EVAL_GRAD, &lml, moments, diagG, &trG, &jit, info))) return rc;
    out5[0] = lml; out5[1] = trG; out5[2] = jit;
    out5[3] = m->pivot_min; out5[4] = m->pivot_max;                    // what mogp_model_pivot_range reports
    if ((rc = mogp_mosm_step_backward(C, Q, D, nscale, cons, dcons, table, moments, diagG, trG, jitter, counts, m->N, twopi, phase_scale, trained, graw)))
        return fail(rc, "mogp_exact_step: bad argument (backward)");
    return MOGP_OK;
}

}  // extern "C"
