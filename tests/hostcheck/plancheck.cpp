// tests/hostcheck/plancheck.cpp — host build of neurec_amd/csrc/spmm_blocked_plan.h.
//
// TEST HARNESS ONLY: runs the lane-group SpMM planner (the very source nrhip_spmm_blocked_plan_create
// calls) with g++ so that tests/test_spmm_plan_cpu.py can check the schedule's invariants without a GPU.
// The product never loads this library.
#include <cstdint>
#include <cstring>
#include <string>
#include "spmm_blocked_plan.h"

namespace {
struct Built {
  nr_plan::Options opt;
  nr_plan::Plan plan;
};
}  // namespace

extern "C" {

// The planner as the C entry runs it, with an explicit workgroup count (n_wg > 0) and the switches as values.
// Returns the status code; on failure the message is copied into err_out.
int pc_plan_create(const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t split_row, int d,
                   int64_t block_bytes, int n_wg, int waves, int seg, int r_max, int p_max, int masked_fast,
                   int wanted_wave, int wanted_nnz_cap, char* err_out, int err_len, void** out) {
  Built* b = new Built();
  nr_plan::Error err;
  int rc = nr_plan::resolve_options(d, waves, seg, r_max, p_max, block_bytes, split_row, n_rows, &b->opt, &err);
  if (rc == nr_plan::kOk) rc = nr_plan::choose_workgroup_count(n_wg, false, n_rows, &b->opt, &err);
  if (rc == nr_plan::kOk) {
    b->opt.masked_fast = masked_fast != 0;
    b->opt.wanted_wave = wanted_wave != 0;
    b->opt.wanted_nnz_cap = wanted_nnz_cap;
    rc = nr_plan::build_plan(indptr, indices, n_rows, b->opt, &b->plan, &err);
  }
  if (rc != nr_plan::kOk) {
    if (err_out && err_len > 0) {
      strncpy(err_out, err.msg.c_str(), (size_t)err_len - 1);
      err_out[err_len - 1] = 0;
    }
    delete b;
    return rc;
  }
  *out = b;
  return rc;
}

void pc_plan_destroy(void* h) { delete (Built*)h; }

int64_t pc_scalar(const void* h, const char* name) {
  const Built* b = (const Built*)h;
  const nr_plan::Plan& p = b->plan;
  const std::string n = name;
#define PC_S(field, value) if (n == #field) return (int64_t)(value)
  PC_S(n_rows, p.n_rows); PC_S(nnz, p.nnz); PC_S(n_wg, p.n_wg); PC_S(n_phases, p.n_phases);
  PC_S(nnz_cap, p.nnz_cap); PC_S(ent_cap, p.ent_cap); PC_S(colmask_ok, p.colmask_ok);
  PC_S(wanted_ok, p.wanted_ok); PC_S(w_ent_cap, p.w_ent_cap); PC_S(w_nnz_cap, p.w_nnz_cap);
  PC_S(w_bitmap_words, p.w_bitmap_words);
  PC_S(ww_ok, p.ww_ok); PC_S(ww_ent_cap, p.ww_ent_cap); PC_S(ww_lds_slots, p.ww_lds_slots);
  PC_S(ww_segments, p.ww_segments);
  PC_S(seg, b->opt.seg); PC_S(r_max, b->opt.r_max); PC_S(p_max, b->opt.p_max); PC_S(waves, b->opt.waves);
  PC_S(split_row, b->opt.split_row);
#undef PC_S
  return INT64_MIN;
}

// a host array by name: its address (valid until pc_plan_destroy) and byte count; 0 when there is no such name
int pc_array(const void* h, const char* name, const void** data, int64_t* bytes) {
  const nr_plan::Plan& p = ((const Built*)h)->plan;
  const std::string n = name;
#define PC_A(field) if (n == #field) { *data = p.field.data(); *bytes = (int64_t)(p.field.size() * sizeof(p.field[0])); return 1; }
  PC_A(wg_row0) PC_A(wg_nrows) PC_A(row_of) PC_A(pk_src) PC_A(pk_dst) PC_A(ent_off) PC_A(cmb_off) PC_A(ent) PC_A(cmb)
  PC_A(wg_nnz) PC_A(w_ent) PC_A(w_cmb) PC_A(w_ent_off) PC_A(w_cmb_off)
  PC_A(ww_off) PC_A(ww_choff) PC_A(ww_lcoff) PC_A(ww_ent) PC_A(ww_gch) PC_A(ww_hub) PC_A(ww_lcmb)
#undef PC_A
  return 0;
}

// the device layout of this plan, carved at address 0: every section's offset and size (bytes + tail padding);
// returns the number of sections, *used gets the end of the last one
int pc_sections(const void* h, int64_t* offsets, int64_t* sizes, int max_sections, int64_t* used) {
  nr_plan::PlanArrays<nr_plan::Int4> dev = {};
  std::vector<nr_plan::Section> s = nr_plan::plan_sections(dev, ((const Built*)h)->plan);
  *used = (int64_t)nr_plan::carve_sections(&s, nullptr);
  for (size_t i = 0; i < s.size() && (int)i < max_sections; ++i) {
    offsets[i] = (int64_t)(uintptr_t)s[i].addr;
    sizes[i] = (int64_t)(s[i].bytes + s[i].pad);
  }
  return (int)s.size();
}

int64_t pc_plan_bytes(int64_t n_rows, int64_t nnz) { return (int64_t)nr_plan::blocked_plan_bytes(n_rows, nnz); }

}  // extern "C"
