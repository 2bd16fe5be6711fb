// Python bindings for the gfx950 HIP kernels.
#include <torch/extension.h>

torch::Tensor floyd_warshall_hip(torch::Tensor w,
                                 c10::optional<torch::Tensor> n_arr);
std::vector<torch::Tensor> decide_hip(
    torch::Tensor sp, torch::Tensor hop, torch::Tensor uds,
    torch::Tensor servers, torch::Tensor src, torch::Tensor mask,
    torch::Tensor ul, torch::Tensor dl,
    c10::optional<torch::Tensor> explore, c10::optional<torch::Tensor> rng,
    long prob);
std::vector<torch::Tensor> walk_eval_hip(
    torch::Tensor sp, torch::Tensor src, torch::Tensor dst,
    torch::Tensor mask, torch::Tensor rate, torch::Tensor ul,
    torch::Tensor dl, torch::Tensor adj_indptr, torch::Tensor adj_idx,
    torch::Tensor adj_link, torch::Tensor conf_indptr,
    torch::Tensor conf_base, torch::Tensor conf_cols, torch::Tensor rates,
    torch::Tensor bw, torch::Tensor edges, torch::Tensor T_arr,
    torch::Tensor E_arr, torch::Tensor n_arr, long H,
    long fp_iters, c10::optional<torch::Tensor> overflow_total);
std::vector<torch::Tensor> critic_hip(
    torch::Tensor route_links, torch::Tensor nhop, torch::Tensor vedge_dst,
    torch::Tensor mask, torch::Tensor rate, torch::Tensor ul,
    torch::Tensor dl, torch::Tensor conf_indptr, torch::Tensor conf_base,
    torch::Tensor conf_cols, torch::Tensor rates, torch::Tensor bw_comp,
    torch::Tensor E_arr, torch::Tensor T_arr, long Ee, long iters,
    double cap, c10::optional<torch::Tensor> node_vedge);
std::vector<torch::Tensor> actor_head_fwd_hip(
    torch::Tensor lam_ext, torch::Tensor conf_indptr,
    torch::Tensor conf_base, torch::Tensor conf_cols, torch::Tensor rates,
    torch::Tensor bw_comp, torch::Tensor edges, torch::Tensor node_vedge,
    torch::Tensor T_arr, torch::Tensor E_arr, long N, long iters,
    double cap);
torch::Tensor actor_head_bwd_hip(
    torch::Tensor grad_dist, torch::Tensor lam_ext, torch::Tensor mu_hist,
    torch::Tensor conf_indptr, torch::Tensor conf_base,
    torch::Tensor conf_cols, torch::Tensor rates, torch::Tensor bw_comp,
    torch::Tensor edges, torch::Tensor node_vedge, torch::Tensor T_arr,
    torch::Tensor E_arr, long iters, double cap);
std::vector<torch::Tensor> actor_head_bwd_fused_hip(
    torch::Tensor grad_edge, torch::Tensor dm, torch::Tensor unit_mtx,
    torch::Tensor written, torch::Tensor lam_ext, torch::Tensor mu_hist,
    torch::Tensor conf_indptr, torch::Tensor conf_base,
    torch::Tensor conf_cols, torch::Tensor rates, torch::Tensor bw_comp,
    torch::Tensor edges, torch::Tensor node_vedge, torch::Tensor T_arr,
    torch::Tensor E_arr, long iters, double cap,
    c10::optional<torch::Tensor> critic_loss);
torch::Tensor floyd_warshall_dm_hip(torch::Tensor dm, torch::Tensor adj,
                                    c10::optional<torch::Tensor> n_arr);
void fw_force_inplace(bool on);
long fw_register_rows(long N);
py::dict queue_lds_plan(long N, long E, long Ee, long iters);
py::dict queue_csr_stage(long N, long E, long Ee, long iters);
long queue_csr_bytes(long Eb, long nnz);
void queue_csr_force_global(bool on);
long queue_csr_set_budget(long bytes);

// timeslot.hip
std::vector<torch::Tensor> timeslot_sim_hip(
    torch::Tensor arrivals, torch::Tensor slot_off, torch::Tensor route_links,
    torch::Tensor nhop, torch::Tensor dst, torch::Tensor mask,
    torch::Tensor ul, torch::Tensor dl, torch::Tensor conf_indptr,
    torch::Tensor conf_base, torch::Tensor conf_cols, torch::Tensor rates,
    torch::Tensor bw, torch::Tensor T_arr, torch::Tensor E_arr,
    torch::Tensor n_arr, long warmup, long pool, bool want_trace);
py::dict timeslot_lds_plan(long N, long E, long J);
std::vector<torch::Tensor> timeslot_sim_stats_hip(
    torch::Tensor arrivals, torch::Tensor slot_off, torch::Tensor route_links,
    torch::Tensor nhop, torch::Tensor dst, torch::Tensor mask,
    torch::Tensor ul, torch::Tensor dl, torch::Tensor conf_indptr,
    torch::Tensor conf_base, torch::Tensor conf_cols, torch::Tensor rates,
    torch::Tensor bw, torch::Tensor T_arr, torch::Tensor E_arr,
    torch::Tensor n_arr, long warmup, long pool, bool want_trace,
    torch::Tensor late_after, long nbins);
py::dict timeslot_stats_lds_plan(long N, long E, long J);
std::vector<torch::Tensor> timeslot_sim_mwis_hip(
    torch::Tensor arrivals, torch::Tensor slot_off, torch::Tensor route_links,
    torch::Tensor nhop, torch::Tensor dst, torch::Tensor mask,
    torch::Tensor ul, torch::Tensor dl, torch::Tensor conf_indptr,
    torch::Tensor conf_base, torch::Tensor conf_cols, torch::Tensor rates,
    torch::Tensor bw, torch::Tensor T_arr, torch::Tensor E_arr,
    torch::Tensor n_arr, long warmup, long pool, bool want_trace);
std::vector<torch::Tensor> timeslot_sim_mwis_stats_hip(
    torch::Tensor arrivals, torch::Tensor slot_off, torch::Tensor route_links,
    torch::Tensor nhop, torch::Tensor dst, torch::Tensor mask,
    torch::Tensor ul, torch::Tensor dl, torch::Tensor conf_indptr,
    torch::Tensor conf_base, torch::Tensor conf_cols, torch::Tensor rates,
    torch::Tensor bw, torch::Tensor T_arr, torch::Tensor E_arr,
    torch::Tensor n_arr, long warmup, long pool, bool want_trace,
    torch::Tensor late_after, long nbins);
py::dict timeslot_mwis_lds_plan(long N, long E, long J, bool stats);

// step_glue.hip
std::vector<torch::Tensor> cheb_pack_params_hip(
    std::vector<torch::Tensor> params);
void cheb_reduce_grads_hip(torch::Tensor dW, torch::Tensor db,
                           std::vector<std::vector<int64_t>> shapes,
                           torch::Tensor flat_out,
                           std::vector<int64_t> offsets, bool accumulate);
torch::Tensor cheb_features_hip(
    torch::Tensor sources, torch::Tensor rates, torch::Tensor ul,
    torch::Tensor mask, torch::Tensor node_vedge, torch::Tensor comp_mask,
    torch::Tensor f_self_loop, torch::Tensor f_rate,
    torch::Tensor f_as_server);
std::vector<torch::Tensor> episode_summary_hip(torch::Tensor delay_emp,
                                               torch::Tensor mask,
                                               torch::Tensor T_arr);
std::vector<torch::Tensor> jobs_from_draws_hip(
    torch::Tensor scores_raw, torch::Tensor r_nj, torch::Tensor r_rates,
    torch::Tensor mobile_mask, double arrival_scale);

std::vector<torch::Tensor> cheb_fwd_hip(
    torch::Tensor x, torch::Tensor W, torch::Tensor bias,
    torch::Tensor ext_indptr, torch::Tensor ext_base, torch::Tensor ext_cols,
    long max_nnz);
std::vector<torch::Tensor> cheb_bwd_hip(
    torch::Tensor dlam, torch::Tensor acts, torch::Tensor t1s,
    torch::Tensor W, torch::Tensor ext_indptr, torch::Tensor ext_base,
    torch::Tensor ext_cols, long max_nnz);

std::vector<torch::Tensor> cheb_bwd_hip_mask(
    torch::Tensor dlam, torch::Tensor acts, torch::Tensor t1s,
    torch::Tensor W, torch::Tensor ext_indptr, torch::Tensor ext_base,
    torch::Tensor ext_cols, long max_nnz, long stage_mask);
std::vector<torch::Tensor> cheb_kn_fwd_hip(
    torch::Tensor x, torch::Tensor W, torch::Tensor bias,
    torch::Tensor ext_indptr, torch::Tensor ext_base, torch::Tensor ext_cols,
    long max_nnz);
std::vector<torch::Tensor> cheb_kn_bwd_hip(
    torch::Tensor dlam, torch::Tensor acts, torch::Tensor tks,
    torch::Tensor W, torch::Tensor ext_indptr, torch::Tensor ext_base,
    torch::Tensor ext_cols, long max_nnz);
bool cheb_fits_lds(long Ee, long K);
py::dict cheb_lds_plan_py(long Ee, long K, long max_nnz);
void cheb_force_full_width(bool on);
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, bool>
cheb_fwd_edge_hip(torch::Tensor x, torch::Tensor W, torch::Tensor bias,
                  torch::Tensor ext_indptr, torch::Tensor ext_base,
                  torch::Tensor ext_cols, long max_nnz, long out_width);
std::vector<torch::Tensor> cheb_bwd_edge_hip(
    torch::Tensor dlam, torch::Tensor x, torch::Tensor lam,
    torch::Tensor acts, torch::Tensor t1s, torch::Tensor W,
    torch::Tensor ext_indptr, torch::Tensor ext_base,
    torch::Tensor ext_cols, long max_nnz, bool edge);
std::vector<torch::Tensor> cheb_bwd_edge_hip_mask(
    torch::Tensor dlam, torch::Tensor x, torch::Tensor lam,
    torch::Tensor acts, torch::Tensor t1s, torch::Tensor W,
    torch::Tensor ext_indptr, torch::Tensor ext_base,
    torch::Tensor ext_cols, long max_nnz, bool edge, long stage_mask);

std::vector<torch::Tensor> cheb_large_fwd_hip(
    torch::Tensor x, torch::Tensor W, torch::Tensor bias,
    torch::Tensor ext_indptr, torch::Tensor ext_base,
    torch::Tensor ext_cols);
std::vector<torch::Tensor> cheb_large_bwd_hip(
    torch::Tensor dlam, torch::Tensor acts, torch::Tensor W,
    torch::Tensor ext_indptr, torch::Tensor ext_base,
    torch::Tensor ext_cols);
void fused_adam_hip(torch::Tensor p, torch::Tensor g, torch::Tensor m,
                    torch::Tensor v, torch::Tensor seg, torch::Tensor step,
                    double scale, double lr, double beta1, double beta2,
                    double eps, bool constraints,
                    c10::optional<torch::Tensor> ticket);
void adam_force_single_block(bool on);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.def("floyd_warshall", &floyd_warshall_hip);
    m.def("decide", &decide_hip);
    m.def("walk_eval", &walk_eval_hip, py::arg("sp"), py::arg("src"),
          py::arg("dst"), py::arg("mask"), py::arg("rate"), py::arg("ul"),
          py::arg("dl"), py::arg("adj_indptr"), py::arg("adj_idx"),
          py::arg("adj_link"), py::arg("conf_indptr"), py::arg("conf_base"),
          py::arg("conf_cols"), py::arg("rates"), py::arg("bw"),
          py::arg("edges"), py::arg("T_arr"), py::arg("E_arr"),
          py::arg("n_arr"), py::arg("H"), py::arg("fp_iters"),
          py::arg("overflow_total") = py::none());
    m.def("critic", &critic_hip, py::arg("route_links"), py::arg("nhop"),
          py::arg("vedge_dst"), py::arg("mask"), py::arg("rate"),
          py::arg("ul"), py::arg("dl"), py::arg("conf_indptr"),
          py::arg("conf_base"), py::arg("conf_cols"), py::arg("rates"),
          py::arg("bw_comp"), py::arg("E_arr"), py::arg("T_arr"),
          py::arg("Ee"), py::arg("iters"), py::arg("cap"),
          py::arg("node_vedge") = py::none());
    m.def("actor_head_fwd", &actor_head_fwd_hip);
    m.def("actor_head_bwd", &actor_head_bwd_hip);
    m.def("actor_head_bwd_fused", &actor_head_bwd_fused_hip,
          py::arg("grad_edge"), py::arg("dm"), py::arg("unit_mtx"),
          py::arg("written"), py::arg("lam_ext"), py::arg("mu_hist"),
          py::arg("conf_indptr"), py::arg("conf_base"), py::arg("conf_cols"),
          py::arg("rates"), py::arg("bw_comp"), py::arg("edges"),
          py::arg("node_vedge"), py::arg("T_arr"), py::arg("E_arr"),
          py::arg("iters"), py::arg("cap"),
          py::arg("critic_loss") = py::none());
    m.def("floyd_warshall_dm", &floyd_warshall_dm_hip);
    m.def("fw_force_inplace", &fw_force_inplace);
    m.def("fw_register_rows", &fw_register_rows);
    m.def("cheb_pack_params", &cheb_pack_params_hip);
    m.def("cheb_reduce_grads", &cheb_reduce_grads_hip);
    m.def("cheb_features", &cheb_features_hip);
    m.def("episode_summary", &episode_summary_hip);
    m.def("jobs_from_draws", &jobs_from_draws_hip);
    m.def("queue_lds_plan", &queue_lds_plan);
    m.def("queue_csr_stage", &queue_csr_stage);
    m.def("queue_csr_bytes", &queue_csr_bytes);
    m.def("queue_csr_force_global", &queue_csr_force_global);
    m.def("queue_csr_set_budget", &queue_csr_set_budget);
    m.def("timeslot_sim", &timeslot_sim_hip);
    m.def("timeslot_lds_plan", &timeslot_lds_plan);
    m.def("timeslot_sim_stats", &timeslot_sim_stats_hip);
    m.def("timeslot_stats_lds_plan", &timeslot_stats_lds_plan);
    m.def("timeslot_sim_mwis", &timeslot_sim_mwis_hip);
    m.def("timeslot_sim_mwis_stats", &timeslot_sim_mwis_stats_hip);
    m.def("timeslot_mwis_lds_plan", &timeslot_mwis_lds_plan);
    m.def("cheb_fwd", &cheb_fwd_hip);
    m.def("cheb_bwd", &cheb_bwd_hip);
    m.def("cheb_bwd_ablate", &cheb_bwd_hip_mask);
    m.def("cheb_force_full_width", &cheb_force_full_width);
    m.def("cheb_fwd_edge", &cheb_fwd_edge_hip);
    m.def("cheb_bwd_edge", &cheb_bwd_edge_hip);
    m.def("cheb_bwd_edge_ablate", &cheb_bwd_edge_hip_mask);
    m.def("cheb_kn_fwd", &cheb_kn_fwd_hip);
    m.def("cheb_kn_bwd", &cheb_kn_bwd_hip);
    m.def("cheb_fits_lds", &cheb_fits_lds);
    m.def("cheb_lds_plan", &cheb_lds_plan_py);
    m.def("fused_adam", &fused_adam_hip, py::arg("p"), py::arg("g"),
          py::arg("m"), py::arg("v"), py::arg("seg"), py::arg("step"),
          py::arg("scale"), py::arg("lr"), py::arg("beta1"),
          py::arg("beta2"), py::arg("eps"), py::arg("constraints"),
          py::arg("ticket") = py::none());
    m.def("adam_force_single_block", &adam_force_single_block);
    m.def("cheb_large_fwd", &cheb_large_fwd_hip);
    m.def("cheb_large_bwd", &cheb_large_bwd_hip);
}
