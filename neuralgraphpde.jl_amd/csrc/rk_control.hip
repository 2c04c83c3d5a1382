// rk_control.hip -- host only, no device call: the step-size controller of adaptive Tsit5 (docs/src/tutorials/graph_node.md:80-81
// `NeuralODE(node_chain; ..., reltol = 1e-3, abstol = 1e-3)`, VMH.md:87 `NeuralODE(gnn, tspan, Tsit5(); saveat, reltol, abstol)`).
// The policy is OrdinaryDiffEq's: ode_determine_initdt for the starting step (order 5) and the PI controller with Tsit5's defaults.
// The caller steps (forms the stages, the error estimate with ngpde_rk_error_norm, reads it back) and asks this code what to do next.
#include <cmath>

#include "common.h"

namespace ngpde {
namespace {

constexpr double kBeta1 = 7.0 / 50.0, kBeta2 = 2.0 / 25.0, kGamma = 9.0 / 10.0, kQmin = 1.0 / 5.0, kQmax = 10.0, kQoldInit = 1e-4;

// t of the next stop: the next save point t0 + k saveat (the last one is t_end itself), or t_end
double next_stop(const ngpde_rk_control_t *s) {
  if (s->saveat > 0.0 && s->next_save < s->n_save) return s->t0 + (double)s->next_save * s->saveat;
  return s->t_end;
}

// the attempt after this one: the proposal capped by dtmax, then cut to land on the next stop
int32_t propose(ngpde_rk_control_t *s, double dt_next) {
  const double dt = dt_next < s->dtmax ? dt_next : s->dtmax;
  if (!(dt >= s->dtmin)) {      // (a NaN step fails here too)
    s->done = -1;
    return fail(NGPDE_ERR_STATE, "adaptive step size: dt = %.17g fell below dtmin = %.17g at t = %.17g", dt, s->dtmin, s->t);
  }
  const double stop = next_stop(s);
  if (dt >= stop - s->t) {
    s->dt = stop - s->t;
    s->lands = 1;
  } else {
    s->dt = dt;
    s->lands = 0;
  }
  return NGPDE_OK;
}

// Tsit5's free 4th-order interpolant (Tsitouras 2011, the form OrdinaryDiffEq's Tsit5 dense output uses):
// b_i(theta) = r_i1 theta + r_i2 theta^2 + r_i3 theta^3 + r_i4 theta^4 over the seven stages, the seventh being f(u_new)
constexpr double kTsit5Interp[7][4] = {
    {1.0, -2.763706197274826, 2.9132554618219126, -1.0530884977290216},
    {0.0, 0.13169999999999998, -0.2234, 0.1017},
    {0.0, 3.9302962368947516, -5.941033872131505, 2.490627285651253},
    {0.0, -12.411077166933676, 30.33818863028232, -16.548102889244902},
    {0.0, 37.50931341651104, -88.1789048947664, 47.37952196281928},
    {0.0, -27.896526289197286, 65.09189467479366, -34.87065786149661},
    {0.0, 1.5, -4.0, 2.5},
};

}  // namespace
}  // namespace ngpde

using namespace ngpde;

extern "C" {

int32_t ngpde_rk_tsit5_interp_coefs(double theta, double dt, double *coefs) {
  NGPDE_REQUIRE(coefs, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_rk_tsit5_interp_coefs: NULL argument");
  NGPDE_REQUIRE(theta >= 0.0 && theta <= 1.0, NGPDE_ERR_INVALID_ARGUMENT,
                "ngpde_rk_tsit5_interp_coefs: 0 <= theta <= 1 required (got %g)", theta);
  NGPDE_REQUIRE(std::isfinite(dt), NGPDE_ERR_INVALID_ARGUMENT, "ngpde_rk_tsit5_interp_coefs: dt must be finite (got %g)", dt);
  for (int i = 0; i < 7; ++i) {
    const double *r = kTsit5Interp[i];
    coefs[i] = dt * (theta * (r[0] + theta * (r[1] + theta * (r[2] + theta * r[3]))));
  }
  return NGPDE_OK;
}

int32_t ngpde_rk_control_init(ngpde_rk_control_t *s, double t0, double t_end, double dt, double dtmax, double saveat, int64_t maxiters) {
  NGPDE_REQUIRE(s, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_rk_control_init: NULL state");
  NGPDE_REQUIRE(std::isfinite(t0) && std::isfinite(t_end) && t_end > t0, NGPDE_ERR_INVALID_ARGUMENT,
                "ngpde_rk_control_init: a finite tspan with t_end > t0 required (got %g, %g)", t0, t_end);
  const double span = t_end - t0;
  NGPDE_REQUIRE(std::isfinite(dt) && std::isfinite(dtmax) && std::isfinite(saveat) && saveat >= 0.0, NGPDE_ERR_INVALID_ARGUMENT,
                "ngpde_rk_control_init: dt, dtmax and saveat must be finite, saveat >= 0 (got %g, %g, %g)", dt, dtmax, saveat);
  int64_t n_save = 0;
  if (saveat > 0.0) {
    const double n = std::nearbyint(span / saveat);
    NGPDE_REQUIRE(n >= 1.0 && n <= 1e9 && std::fabs(n * saveat - span) <= 1e-6 * span, NGPDE_ERR_INVALID_ARGUMENT,
                  "ngpde_rk_control_init: saveat = %g must divide tspan (%g, %g) into whole intervals", saveat, t0, t_end);
    n_save = (int64_t)n;
  }
  *s = ngpde_rk_control_t{};
  s->t0 = t0;
  s->t = t0;
  s->t_end = t_end;
  s->dtmax = dtmax > 0.0 ? dtmax : span;
  s->dtmin = 1e-12 * span;
  s->saveat = saveat;
  s->n_save = n_save;
  s->next_save = 1;
  s->maxiters = maxiters > 0 ? maxiters : 100000;
  s->qold = kQoldInit;
  if (dt > 0.0) return propose(s, dt);
  return NGPDE_OK;     // dt <= 0: ngpde_rk_control_trial_dt / _initial_dt choose it
}

int32_t ngpde_rk_control_trial_dt(const ngpde_rk_control_t *s, double d0, double d1, double *dt0) {
  NGPDE_REQUIRE(s && dt0, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_rk_control_trial_dt: NULL argument");
  NGPDE_REQUIRE(std::isfinite(d0) && std::isfinite(d1), NGPDE_ERR_STATE,
                "ngpde_rk_control_trial_dt: the state or the right-hand side at t = %.17g is not finite (|u0/sk| = %g, |f0/sk| = %g)",
                s->t, d0, d1);
  double d = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * (d0 / d1);
  *dt0 = d < s->dtmax ? d : s->dtmax;
  return NGPDE_OK;
}

int32_t ngpde_rk_control_initial_dt(ngpde_rk_control_t *s, double d0, double d1, double norm_df) {
  double dt0 = 0.0;
  const int32_t st = ngpde_rk_control_trial_dt(s, d0, d1, &dt0);
  if (st) return st;
  NGPDE_REQUIRE(std::isfinite(norm_df), NGPDE_ERR_STATE,
                "ngpde_rk_control_initial_dt: the right-hand side after the trial step from t = %.17g is not finite", s->t);
  const double d2 = norm_df / dt0;
  const double m = d1 > d2 ? d1 : d2;
  double dt1;
  if (m <= 1e-15) dt1 = 1e-6 > 1e-3 * dt0 ? 1e-6 : 1e-3 * dt0;
  else dt1 = std::pow(0.01 / m, 1.0 / 5.0);
  double dt = 100.0 * dt0;
  if (dt1 < dt) dt = dt1;
  if (s->dtmax < dt) dt = s->dtmax;
  return propose(s, dt);
}

int32_t ngpde_rk_control_step(ngpde_rk_control_t *s, double eest, int32_t *action) {
  NGPDE_REQUIRE(s && action, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_rk_control_step: NULL argument");
  NGPDE_REQUIRE(s->done == 0, NGPDE_ERR_STATE, "ngpde_rk_control_step: the solve has %s", s->done > 0 ? "ended" : "failed");
  NGPDE_REQUIRE(s->dt > 0.0, NGPDE_ERR_STATE, "ngpde_rk_control_step: no step size yet (ngpde_rk_control_initial_dt)");
  s->nattempt += 1;
  if (s->nattempt > s->maxiters) {
    s->done = -1;
    return fail(NGPDE_ERR_STATE, "adaptive step size: maxiters = %lld attempts reached at t = %.17g", (long long)s->maxiters, s->t);
  }
  s->eest = eest;
  s->saved = 0;
  double dt_next;
  if (!std::isfinite(eest)) {         // NaN / Inf in the attempt: a reject by the factor qmin
    dt_next = s->dt * kQmin;
    s->nreject += 1;
    *action = NGPDE_RK_REJECT;
  } else {
    double q;
    if (eest == 0.0) {
      q = 1.0 / kQmax;
    } else {
      s->q11 = std::pow(eest, kBeta1);
      q = s->q11 / std::pow(s->qold, kBeta2) / kGamma;
      q = q < 1.0 / kQmax ? 1.0 / kQmax : (q > 1.0 / kQmin ? 1.0 / kQmin : q);
    }
    if (eest <= 1.0) {
      s->qold = eest > kQoldInit ? eest : kQoldInit;
      dt_next = s->dt / q;
      const double stop = next_stop(s);
      s->t = s->lands ? stop : s->t + s->dt;     // landing: the stop itself, not t + dt
      s->naccept += 1;
      *action = NGPDE_RK_ACCEPT;
      if (s->lands) {
        if (s->saveat > 0.0) {
          s->saved = 1;
          s->next_save += 1;
        }
        if (stop == s->t_end) {
          s->done = 1;
          *action = NGPDE_RK_DONE;
          return NGPDE_OK;
        }
      }
    } else {
      const double r = s->q11 / kGamma;
      dt_next = s->dt / (1.0 / kQmin < r ? 1.0 / kQmin : r);
      s->nreject += 1;
      *action = NGPDE_RK_REJECT;
    }
  }
  return propose(s, dt_next);
}

}  // extern "C"
