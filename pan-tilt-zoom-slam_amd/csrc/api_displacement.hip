// The projection-centre displacement of the C-ABI (include/ptzba.h ptzba_set_displacement).  The six
// constants live in the handle; every launch that projects (K1's two kernels, the record-order residual, the
// covariance's residual scale) picks its displaced instantiation while they are set.
#include <cmath>

#include "ba_ctx.h"

using namespace ptzba;

int ptzba_set_displacement(ptzba_handle h, const double* displacement6) {
  if (!h || !h->have_problem) return fail("no problem set");
  if (h->trial_open || h->scal_deferred)
    return fail("ptzba_set_displacement: an LM trial is pending (accept or reject it first; the call runs between "
                "solves)");
  bool any = false;
  if (displacement6)
    for (int k = 0; k < 6; ++k) {
      if (!std::isfinite(displacement6[k])) return fail("ptzba_set_displacement: non-finite entry %d", k);
      any = any || displacement6[k] != 0.0;
    }
  if (any && (h->dist_mode || h->dist_world > 1 || h->has_exchange() || h->ext_exchange || h->scal_exported))
    return fail("ptzba_set_displacement: single rank only (the handle is sharded, has a communicator / hook attached "
                "or runs a caller-side exchange)");
  // (the constants travel by value in each launch's arguments: queued work keeps the ones it was launched with)
  for (int k = 0; k < 6; ++k) h->disp[k] = any ? displacement6[k] : 0.0;
  h->displaced = any;
  return 0;
}

int ptzba_displacement_info(ptzba_handle h, double* out8) {
  if (!h || !h->have_problem) return fail("no problem set");
  if (!out8) return fail("ptzba_displacement_info: null output");
  out8[0] = h->displaced ? 1.0 : 0.0;
  for (int k = 0; k < 6; ++k) out8[1 + k] = h->disp[k];
  out8[7] = 0.0;
  return 0;
}
