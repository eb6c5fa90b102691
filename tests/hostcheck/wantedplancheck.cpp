// g++ build of neurec_amd/csrc/spmm_wanted_plan.h for tests/test_spmm_wanted_plan_cpu.py: the per-batch item lists
// of the planned batch-rows hop, made by the header's host statement (plan_batch) on the hub records of the real
// lane-group planner (nr_plan::wanted_wave_schedule).
#include "spmm_wanted_plan.h"

extern "C" {

int64_t wp_stride(const int64_t* indptr, int64_t n_rows, int batch) {
  return nr_wplan::stride_of(nr_wplan::slot_profile(indptr, n_rows), batch);
}

int64_t wp_items_bound(const int64_t* indptr, int64_t n_rows, int batch) {
  return nr_wplan::items_bound(nr_wplan::slot_profile(indptr, n_rows), batch);
}

// out: stride records of 4 int32; returns the item count (-1: refused); *n_hubs / hubs_out (optional, room for
// n_rows records): the planner's hub records {row, first partial slot, segments, chunks}
int64_t wp_plan_batch(const int64_t* indptr, int64_t n_rows, const uint64_t* keys, int n_keys, int64_t stride,
                      int32_t* out, int32_t* hubs_out, int64_t* n_hubs) {
  nr_plan::Options opt;
  opt.d = 64; opt.waves = 16; opt.seg = nr_wplan::kSeg; opt.r_max = nr_plan::kRMaxDefault; opt.p_max = nr_plan::kPMaxDefault;
  opt.block_bytes = (int64_t)1 << 40; opt.split_row = 0; opt.n_wg = 256;
  nr_plan::Plan h;
  h.n_rows = n_rows;
  h.nnz = indptr[n_rows];
  h.n_wg = opt.n_wg;
  nr_plan::wanted_wave_schedule(indptr, opt, &h);
  if (n_hubs) *n_hubs = (int64_t)h.ww_hub.size();
  if (hubs_out)
    for (size_t i = 0; i < h.ww_hub.size(); ++i) {
      hubs_out[4 * i] = h.ww_hub[i].x; hubs_out[4 * i + 1] = h.ww_hub[i].y;
      hubs_out[4 * i + 2] = h.ww_hub[i].z; hubs_out[4 * i + 3] = h.ww_hub[i].w;
    }
  return nr_wplan::plan_batch(indptr, h.ww_hub, keys, n_keys, stride, (nr_plan::Int4*)out);
}

}  // extern "C"
