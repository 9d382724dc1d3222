// rsx_es.hip -- the kernels and launchers of ONE element size: compiled once per size with
// -DRSX_ES=<bytes> (radix_sort_amd/_build.py), so that the eight sizes build in parallel and a
// tuning variant of one size relinks in seconds.
#ifndef RSX_ES
#error "compile with -DRSX_ES=<element bytes>"
#endif
#include "rsx_launch_impl.hpp"

namespace rsxh {
template <>
const EsLaunchers& es_launchers<RSX_ES>() {
    static const EsLaunchers t = {launch_segment_sort<RSX_ES>, launch_hist<RSX_ES>, launch_hist2<RSX_ES>, launch_wideplan<RSX_ES>, launch_count16top<RSX_ES>,
                                  launch_marginal16<RSX_ES>, launch_bucket16<RSX_ES>, launch_mid_split<RSX_ES>, launch_bucket_sort<RSX_ES>,
                                  launch_sweep<RSX_ES>, launch_small_sort<RSX_ES>, launch_segcopy<RSX_ES>, launch_segment_pairs<RSX_ES>, launch_topk<RSX_ES>};
    return t;
}
}  // namespace rsxh
