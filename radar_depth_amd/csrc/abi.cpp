// The C ABI's prototype table: every entry point of include/radar_depth_hip.h as "<name> <ret>:<args>", one character per type,
// derived by the compiler from the declarations (rd_abi_entries / rd_abi_entry).  Bindings set their foreign-function prototypes from
// it instead of restating them (radar_depth_amd/_lib.py).
//   p pointer, s pointer to char, f float, d double; b h i l / B H I L: signed / unsigned integer of 1, 2, 4, 8 bytes.
// A new entry point is declared in the header, defined in its source file and named ONCE below (tests/test_abi_host.py compares the
// list with the header).
#include <string>
#include <type_traits>

#include "common.h"

namespace {

template <typename T>
constexpr char code() {
    if constexpr (std::is_pointer_v<T>) {
        static_assert(!std::is_function_v<std::remove_pointer_t<T>>, "the C ABI takes no function pointers");
        return std::is_same_v<std::remove_cv_t<std::remove_pointer_t<T>>, char> ? 's' : 'p';
    } else if constexpr (std::is_floating_point_v<T>) {
        static_assert(std::is_same_v<T, float> || std::is_same_v<T, double>, "the C ABI's floating types are float and double");
        return std::is_same_v<T, float> ? 'f' : 'd';
    } else {
        static_assert(std::is_integral_v<T> && (sizeof(T) == 1 || sizeof(T) == 2 || sizeof(T) == 4 || sizeof(T) == 8),
                      "the C ABI passes pointers, integers, float and double only");
        return (std::is_signed_v<T> ? "bhxixxxl" : "BHxIxxxL")[sizeof(T) - 1];
    }
}

template <typename R, typename... A>
std::string signature(const char* name, R (*)(A...)) {
    return std::string(name) + ' ' + code<R>() + ':' + std::string{code<A>()...};
}

#define RD_ABI_ENTRIES \
    X(rd_abi_entries) \
    X(rd_abi_entry) \
    X(rd_abi_version) \
    X(rd_act_gate_t) \
    X(rd_adam_prepare) \
    X(rd_adam_step) \
    X(rd_allreduce_bucket) \
    X(rd_berhu_workspace_floats) \
    X(rd_bilinear_bwd) \
    X(rd_bilinear_fwd) \
    X(rd_bn_act) \
    X(rd_bn_act_p) \
    X(rd_bn_act_t) \
    X(rd_bn_bwd_apply) \
    X(rd_bn_bwd_apply_p) \
    X(rd_bn_bwd_apply_t) \
    X(rd_bn_bwd_apply_x) \
    X(rd_bn_bwd_apply_x2) \
    X(rd_bn_bwd_apply_x2_p) \
    X(rd_bn_bwd_apply_x2_t) \
    X(rd_bn_bwd_apply_x_p) \
    X(rd_bn_bwd_apply_x_t) \
    X(rd_bn_bwd_reduce) \
    X(rd_bn_bwd_reduce_t) \
    X(rd_bn_bwd_reduce_x) \
    X(rd_bn_bwd_reduce_x2) \
    X(rd_bn_bwd_reduce_x2_t) \
    X(rd_bn_bwd_reduce_x_t) \
    X(rd_bn_bwd_tiles) \
    X(rd_bn_eval_coeffs) \
    X(rd_bn_eval_coeffs_batched) \
    X(rd_bn_finalize) \
    X(rd_bn_stats) \
    X(rd_bn_stats_t) \
    X(rd_bn_stats_tiles) \
    X(rd_bnact_maxpool_bwd) \
    X(rd_bnact_maxpool_bwd_apply_t) \
    X(rd_bnact_maxpool_bwd_stats) \
    X(rd_bnact_maxpool_bwd_stats_t) \
    X(rd_bnact_maxpool_bwd_t) \
    X(rd_bnact_maxpool_bwd_tiles) \
    X(rd_bnact_maxpool_fwd) \
    X(rd_bnact_maxpool_fwd_p) \
    X(rd_bnact_maxpool_fwd_t) \
    X(rd_broadcast) \
    X(rd_clock_probe) \
    X(rd_comm_destroy) \
    X(rd_comm_init) \
    X(rd_comm_rank) \
    X(rd_comm_unique_id) \
    X(rd_comm_world) \
    X(rd_conv16_split) \
    X(rd_conv16_split_supported) \
    X(rd_debug_poison_lds) \
    X(rd_depth_metrics) \
    X(rd_depth_metrics_frames) \
    X(rd_depth_metrics_frames_workspace_floats) \
    X(rd_depth_metrics_multidist) \
    X(rd_depth_metrics_multidist_workspace_floats) \
    X(rd_device_info) \
    X(rd_event_create) \
    X(rd_event_destroy) \
    X(rd_event_record) \
    X(rd_fill) \
    X(rd_gconv) \
    X(rd_gconv_bf16) \
    X(rd_gconv_bf16_plan_info) \
    X(rd_gconv_bf16_plan_info_t) \
    X(rd_gconv_bf16_stat_tiles) \
    X(rd_gconv_bf16_stat_tiles_t) \
    X(rd_gconv_bf16_t) \
    X(rd_gconv_bf16_trace_read) \
    X(rd_gconv_bf16p_plan_all) \
    X(rd_gconv_bnbwd) \
    X(rd_gconv_bnbwd_supported) \
    X(rd_gconv_fused) \
    X(rd_gconv_occupancy) \
    X(rd_gconv_plan_info) \
    X(rd_gconv_plan_state) \
    X(rd_gconv_split) \
    X(rd_gconv_split_bnbwd) \
    X(rd_gconv_split_bnbwd_supported) \
    X(rd_gconv_split_plan_all) \
    X(rd_gconv_split_plan_info) \
    X(rd_gconv_split_pre) \
    X(rd_gconv_split_pre_bnbwd) \
    X(rd_gconv_split_pre_plan_info) \
    X(rd_gconv_split_pre_preferred) \
    X(rd_gconv_split_pre_stat_tiles) \
    X(rd_gconv_split_pre_supported) \
    X(rd_gconv_split_slot_map) \
    X(rd_gconv_split_stat_tiles) \
    X(rd_gconv_split_supported) \
    X(rd_gconv_split_trace_read) \
    X(rd_gconv_stat_tiles) \
    X(rd_gconv_stat_tiles_ws) \
    X(rd_gconv_trace_read) \
    X(rd_gconv_tune_candidates) \
    X(rd_gconv_tune_commit) \
    X(rd_gconv_tune_pin) \
    X(rd_gconv_workspace_floats) \
    X(rd_gconv_ws) \
    X(rd_gemm_taps_split) \
    X(rd_gemm_taps_split_plan_info) \
    X(rd_gemm_taps_split_preferred) \
    X(rd_gemm_taps_split_stat_tiles) \
    X(rd_gemm_taps_split_supported) \
    X(rd_grad_sumsq) \
    X(rd_grad_sumsq_partials) \
    X(rd_graph_begin) \
    X(rd_graph_destroy) \
    X(rd_graph_end) \
    X(rd_graph_launch) \
    X(rd_head_conv_bwd) \
    X(rd_head_conv_bwd_t) \
    X(rd_head_conv_bwd_workspace_floats) \
    X(rd_head_conv_dgrad_t) \
    X(rd_head_conv_fwd) \
    X(rd_head_conv_fwd_t) \
    X(rd_head_conv_wgrad_t) \
    X(rd_kitti_decode) \
    X(rd_kitti_encode) \
    X(rd_kitti_error_image) \
    X(rd_kitti_errors) \
    X(rd_kitti_interpolate) \
    X(rd_kitti_stats_update) \
    X(rd_kitti_workspace_bytes) \
    X(rd_l1_total) \
    X(rd_last_error) \
    X(rd_lidar_radar_sparsify) \
    X(rd_lidar_sparsify_workspace_bytes) \
    X(rd_loss_tiles) \
    X(rd_masked_berhu_bwd) \
    X(rd_masked_berhu_sums) \
    X(rd_masked_berhu_sums_metrics) \
    X(rd_masked_l1_bwd) \
    X(rd_masked_l1_sums) \
    X(rd_masked_l1_sums_metrics) \
    X(rd_masked_l2_bwd) \
    X(rd_masked_l2_sums) \
    X(rd_masked_l2_sums_metrics) \
    X(rd_meter_update) \
    X(rd_meter_update_multidist) \
    X(rd_nchw_to_nhwc) \
    X(rd_nhwc_to_nchw) \
    X(rd_optable_add) \
    X(rd_optable_create) \
    X(rd_optable_destroy) \
    X(rd_optable_entry_args) \
    X(rd_optable_run) \
    X(rd_optable_run_mt) \
    X(rd_optable_set_word) \
    X(rd_optable_size) \
    X(rd_pack_chunk) \
    X(rd_pack_weights) \
    X(rd_pack_weights_batched) \
    X(rd_pack_weights_bf16) \
    X(rd_pnp_update) \
    X(rd_radar_filter) \
    X(rd_radar_filter_points) \
    X(rd_radar_index_map) \
    X(rd_render_rows) \
    X(rd_render_workspace_bytes) \
    X(rd_sgd_step) \
    X(rd_sgd_step_clip) \
    X(rd_smooth_bwd) \
    X(rd_smooth_fwd) \
    X(rd_smooth_workspace_floats) \
    X(rd_split_pieces) \
    X(rd_stage_frames) \
    X(rd_stage_frames_train) \
    X(rd_stage_index_filter_train) \
    X(rd_stage_index_filter_val) \
    X(rd_stage_train_workspace_bytes) \
    X(rd_stem_dgrad_channel) \
    X(rd_stem_dgrad_channel_t) \
    X(rd_stem_fwd) \
    X(rd_stem_fwd_bf16) \
    X(rd_stem_fwd_bf16_t) \
    X(rd_stem_fwd_split) \
    X(rd_stem_fwd_t) \
    X(rd_stem_stat_tiles) \
    X(rd_stem_wgrad) \
    X(rd_stem_wgrad_split_bn_t) \
    X(rd_stem_wgrad_split_supported) \
    X(rd_stem_wgrad_split_t) \
    X(rd_stem_wgrad_t) \
    X(rd_stem_wgrad_workspace_floats) \
    X(rd_stream_wait_event) \
    X(rd_uncertainty_total) \
    X(rd_uniform_sparsify) \
    X(rd_wgrad) \
    X(rd_wgrad_bf16) \
    X(rd_wgrad_bf16_plan_info) \
    X(rd_wgrad_bf16_reduce) \
    X(rd_wgrad_bf16_supported) \
    X(rd_wgrad_bf16_t) \
    X(rd_wgrad_bf16_trace_read) \
    X(rd_wgrad_bf16_workspace_floats) \
    X(rd_wgrad_plan_info) \
    X(rd_wgrad_reduce) \
    X(rd_wgrad_reduce_batched) \
    X(rd_wgrad_reduce_job) \
    X(rd_wgrad_split) \
    X(rd_wgrad_split_plan_info) \
    X(rd_wgrad_split_pre) \
    X(rd_wgrad_split_pre_supported) \
    X(rd_wgrad_split_reduce) \
    X(rd_wgrad_split_supported) \
    X(rd_wgrad_split_workspace_floats) \
    X(rd_wgrad_workspace_floats) \
    X(rd_wino_conv3x3) \
    X(rd_wino_conv3x3_bnbwd) \
    X(rd_wino_pack) \
    X(rd_wino_pack_batched) \
    X(rd_wino_pack_blocks) \
    X(rd_wino_packed_bytes) \
    X(rd_wino_preferred) \
    X(rd_wino_stat_tiles) \
    X(rd_wino_supported)

#define X(name) signature(#name, &name),
const std::string kEntries[] = {RD_ABI_ENTRIES};
#undef X
constexpr int kCount = static_cast<int>(sizeof(kEntries) / sizeof(kEntries[0]));

}  // namespace

extern "C" int rd_abi_entries(void) { return kCount; }

extern "C" const char* rd_abi_entry(int i) { return i >= 0 && i < kCount ? kEntries[i].c_str() : nullptr; }
