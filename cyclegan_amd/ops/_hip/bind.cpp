// pybind registration for the gfx950 kernel library.
#include <torch/extension.h>

namespace cyg {
at::Tensor conv2d_fwd(at::Tensor, at::Tensor, c10::optional<at::Tensor>,
                      int64_t, int64_t, int64_t, int64_t, int64_t, bool,
                      int64_t, double);
at::Tensor convt2d_fwd(at::Tensor, at::Tensor, c10::optional<at::Tensor>,
                       int64_t, int64_t, int64_t, int64_t, int64_t, int64_t,
                       double);
std::vector<at::Tensor> conv2d_fwd_stats(at::Tensor, at::Tensor,
                                         c10::optional<at::Tensor>, int64_t,
                                         int64_t, int64_t, int64_t, int64_t,
                                         bool, int64_t, double);
std::vector<at::Tensor> convt2d_fwd_stats(at::Tensor, at::Tensor,
                                          c10::optional<at::Tensor>, int64_t,
                                          int64_t, int64_t, int64_t, int64_t,
                                          int64_t, double);
at::Tensor conv2d_dgrad(at::Tensor, at::Tensor, int64_t, int64_t, int64_t,
                        int64_t, int64_t, int64_t, int64_t, bool);
at::Tensor reflect_dgrad_rowmap(int64_t, int64_t, int64_t, int64_t, int64_t,
                                int64_t, int64_t, int64_t, int64_t, bool,
                                bool);
at::Tensor convt2d_dgrad(at::Tensor, at::Tensor, int64_t, int64_t, int64_t,
                         int64_t, int64_t);
at::Tensor conv2d_wgrad(at::Tensor, at::Tensor, int64_t, int64_t, int64_t,
                        int64_t, int64_t, bool);
void conv2d_wgrad_into(at::Tensor, at::Tensor, int64_t, int64_t, int64_t,
                       int64_t, int64_t, bool, at::Tensor, bool, bool);
void fold_packed_dw_into(at::Tensor, at::Tensor, bool);
at::Tensor mfma_probe(at::Tensor, at::Tensor);
at::Tensor mx_probe(at::Tensor, at::Tensor, int64_t, int64_t);
at::Tensor mx_probe16(at::Tensor, at::Tensor, int64_t, int64_t);
at::Tensor glds_probe(at::Tensor, at::Tensor);
at::Tensor tr_probe(int64_t);
at::Tensor quant_fp8(at::Tensor, at::Tensor);
at::Tensor quant_fp8_d(at::Tensor, at::Tensor, at::Tensor);
void amax_roll(at::Tensor, int64_t);
at::Tensor conv2d_fp8_fwd(at::Tensor, at::Tensor, at::Tensor,
                          c10::optional<at::Tensor>, c10::optional<at::Tensor>,
                          int64_t, int64_t, int64_t, int64_t, int64_t, bool, int64_t, double);
std::vector<at::Tensor> conv2d_fp8_fwd_stats(
    at::Tensor, at::Tensor, at::Tensor, c10::optional<at::Tensor>,
    c10::optional<at::Tensor>, int64_t, int64_t, int64_t, int64_t, int64_t,
    bool, int64_t, double);
std::vector<at::Tensor> instnorm_fwd(at::Tensor, at::Tensor, at::Tensor,
                                     double, int64_t, double,
                                     c10::optional<at::Tensor>,
                                     c10::optional<at::Tensor>,
                                     c10::optional<at::Tensor>, int64_t);
std::vector<at::Tensor> instnorm_fwd_q8(at::Tensor, at::Tensor, at::Tensor,
                                        double, int64_t, double,
                                        c10::optional<at::Tensor>,
                                        c10::optional<at::Tensor>,
                                        c10::optional<at::Tensor>, int64_t,
                                        at::Tensor, at::Tensor);
std::vector<at::Tensor> instnorm_bwd(at::Tensor, at::Tensor, at::Tensor,
                                     at::Tensor, at::Tensor,
                                     c10::optional<at::Tensor>, int64_t,
                                     double, c10::optional<at::Tensor>,
                                     c10::optional<at::Tensor>,
                                     c10::optional<at::Tensor>, bool);
at::Tensor act_bwd(at::Tensor, at::Tensor, int64_t, double);
at::Tensor channel_sum(at::Tensor, c10::optional<at::Tensor>, bool);
at::Tensor reflect_pad_fwd(at::Tensor, int64_t, int64_t, int64_t, int64_t);
at::Tensor reflect_pad_bwd(at::Tensor, int64_t, int64_t, int64_t, int64_t);
at::Tensor persample_loss_fwd(at::Tensor, at::Tensor, bool);
at::Tensor persample_loss_const_fwd(at::Tensor, double, bool);
std::vector<at::Tensor> persample_loss_bwd(at::Tensor, at::Tensor, at::Tensor,
                                           bool, bool, bool);
at::Tensor persample_loss_const_bwd(at::Tensor, double, at::Tensor, bool);
void adam_step_dev(at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor,
                   double, double, double, c10::optional<at::Tensor>);
void adam_ema_step(at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor,
                   double, double, double, double, int64_t, double,
                   c10::optional<at::Tensor>);
void adam_ema_step_dev(at::Tensor, at::Tensor, at::Tensor, at::Tensor,
                       at::Tensor, at::Tensor, double, double, double, double,
                       c10::optional<at::Tensor>);
void shadow_gather(at::Tensor, at::Tensor, at::Tensor);
void shadow_cast(at::Tensor, at::Tensor);
void shadow_transpose(at::Tensor, at::Tensor, at::Tensor, at::Tensor);
void shadow_fold(at::Tensor, at::Tensor, at::Tensor);
void fold_upconv_dw_into(at::Tensor, at::Tensor, bool, bool);
void adam_step(at::Tensor, at::Tensor, at::Tensor, at::Tensor, double, double,
               double, double, int64_t, c10::optional<at::Tensor>);
at::Tensor augment_batch(at::Tensor, at::Tensor, at::Tensor, int64_t, int64_t,
                         at::Tensor);
at::Tensor pool_exchange(at::Tensor, at::Tensor, at::Tensor, at::Tensor);
std::vector<at::Tensor> ssim_fwd(at::Tensor, at::Tensor, int64_t);
at::Tensor ssim_bwd(at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor,
                    at::Tensor);
}  // namespace cyg

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("conv2d_fwd", &cyg::conv2d_fwd);
  m.def("convt2d_fwd", &cyg::convt2d_fwd);
  m.def("conv2d_fwd_stats", &cyg::conv2d_fwd_stats);
  m.def("convt2d_fwd_stats", &cyg::convt2d_fwd_stats);
  m.def("conv2d_dgrad", &cyg::conv2d_dgrad);
  // row order of the direct-fold reflect dgrad as a table (host only)
  m.def("reflect_dgrad_rowmap", &cyg::reflect_dgrad_rowmap, py::arg("B"),
        py::arg("H"), py::arg("W"), py::arg("pt"), py::arg("pb"),
        py::arg("pl"), py::arg("pr"), py::arg("KH"), py::arg("KW"),
        py::arg("trim") = true, py::arg("frame") = false);
  m.def("convt2d_dgrad", &cyg::convt2d_dgrad);
  m.def("conv2d_wgrad", &cyg::conv2d_wgrad);
  // the reduce writes the parameter's true OHWI gradient block `out`
  // (cropped / channel-transposed / added to), e.g. a flat-grad view
  m.def("conv2d_wgrad_into", &cyg::conv2d_wgrad_into, py::arg("x"),
        py::arg("dy"), py::arg("kh"), py::arg("kw"), py::arg("stride"),
        py::arg("pt"), py::arg("pl"), py::arg("reflect"), py::arg("out"),
        py::arg("accumulate"), py::arg("transpose_oi") = false);
  m.def("fold_packed_dw_into", &cyg::fold_packed_dw_into, py::arg("dwp"),
        py::arg("out"), py::arg("accumulate"));
  m.def("mfma_probe", &cyg::mfma_probe);
  m.def("mx_probe", &cyg::mx_probe);
  m.def("mx_probe16", &cyg::mx_probe16);
  m.def("glds_probe", &cyg::glds_probe);
  m.def("tr_probe", &cyg::tr_probe);
  m.def("quant_fp8", &cyg::quant_fp8);
  m.def("quant_fp8_d", &cyg::quant_fp8_d);
  m.def("amax_roll", &cyg::amax_roll);
  m.def("conv2d_fp8_fwd", &cyg::conv2d_fp8_fwd);
  m.def("conv2d_fp8_fwd_stats", &cyg::conv2d_fp8_fwd_stats);
  // trailing optionals keep the short positional forms valid: precomputed
  // slabs (from conv*_fwd_stats) for fwd, beta (mask recompute) for bwd
  m.def("instnorm_fwd", &cyg::instnorm_fwd, py::arg("x"), py::arg("gamma"),
        py::arg("beta"), py::arg("eps"), py::arg("act"), py::arg("slope"),
        py::arg("residual"), py::arg("psum") = py::none(),
        py::arg("psq") = py::none(), py::arg("nslabs") = 0);
  // instnorm_fwd + the e4m3 twin of y for the consuming fp8 conv (slabs
  // are positional here: pass None, None, 0 for the in_reduce route)
  m.def("instnorm_fwd_q8", &cyg::instnorm_fwd_q8, py::arg("x"),
        py::arg("gamma"), py::arg("beta"), py::arg("eps"), py::arg("act"),
        py::arg("slope"), py::arg("residual"), py::arg("psum"),
        py::arg("psq"), py::arg("nslabs"), py::arg("amax_prev"),
        py::arg("amax_cur"));
  m.def("instnorm_bwd", &cyg::instnorm_bwd, py::arg("dy"), py::arg("x"),
        py::arg("gamma"), py::arg("mean"), py::arg("rstd"), py::arg("yact"),
        py::arg("act"), py::arg("slope"), py::arg("beta") = py::none(),
        py::arg("dgamma_out") = py::none(), py::arg("dbeta_out") = py::none(),
        py::arg("accumulate") = false);
  m.def("act_bwd", &cyg::act_bwd);
  m.def("channel_sum", &cyg::channel_sum, py::arg("x"),
        py::arg("out") = py::none(), py::arg("accumulate") = false);
  m.def("reflect_pad_fwd", &cyg::reflect_pad_fwd);
  m.def("reflect_pad_bwd", &cyg::reflect_pad_bwd);
  m.def("persample_loss_fwd", &cyg::persample_loss_fwd);
  m.def("persample_loss_const_fwd", &cyg::persample_loss_const_fwd);
  m.def("persample_loss_bwd", &cyg::persample_loss_bwd);
  m.def("persample_loss_const_bwd", &cyg::persample_loss_const_bwd);
  // trailing `shadow` (all four Adam steps): the bf16 mirror of p that the
  // kernel also writes, bf16(p_new) at each element's own index; None: off
  m.def("adam_step", &cyg::adam_step, py::arg("p"), py::arg("g"),
        py::arg("m"), py::arg("v"), py::arg("lr"), py::arg("b1"),
        py::arg("b2"), py::arg("eps"), py::arg("t"),
        py::arg("shadow") = py::none());
  m.def("adam_step_dev", &cyg::adam_step_dev, py::arg("p"), py::arg("g"),
        py::arg("m"), py::arg("v"), py::arg("lr_t"), py::arg("b1"),
        py::arg("b2"), py::arg("eps"), py::arg("shadow") = py::none());
  // Adam + weight EMA in one pass (p, m, v bitwise as the two above)
  m.def("adam_ema_step", &cyg::adam_ema_step, py::arg("p"), py::arg("g"),
        py::arg("m"), py::arg("v"), py::arg("ema"), py::arg("lr"),
        py::arg("b1"), py::arg("b2"), py::arg("eps"), py::arg("t"),
        py::arg("ema_decay"), py::arg("shadow") = py::none());
  m.def("adam_ema_step_dev", &cyg::adam_ema_step_dev, py::arg("p"),
        py::arg("g"), py::arg("m"), py::arg("v"), py::arg("ema"),
        py::arg("lr_t"), py::arg("b1"), py::arg("b2"), py::arg("eps"),
        py::arg("ema_decay"), py::arg("shadow") = py::none());
  m.def("shadow_gather", &cyg::shadow_gather);
  // mirror refresh outside the optimizer (fp32 masters -> bf16 mirror), and
  // the index-free [Cout,taps,Cin] -> [Cin,taps,Cout] transposes of the
  // dgrad forms over a per-layer table (host copy validated per call)
  m.def("shadow_cast", &cyg::shadow_cast);
  m.def("shadow_transpose", &cyg::shadow_transpose, py::arg("src"),
        py::arg("table"), py::arg("table_dev"), py::arg("dst"));
  // resize-convolution: folded 4x4 forms from the 3x3 masters, and the
  // 4x4 weight gradient unfolded onto the 3x3 master's gradient block
  m.def("shadow_fold", &cyg::shadow_fold);
  m.def("fold_upconv_dw_into", &cyg::fold_upconv_dw_into, py::arg("dv"),
        py::arg("out"), py::arg("accumulate"), py::arg("transposed"));
  m.def("augment_batch", &cyg::augment_batch);
  m.def("pool_exchange", &cyg::pool_exchange);
  // per-sample mean SSIM: [out] or, save_maps 1/2, [out, ay, b, c(, ax)]
  m.def("ssim_fwd", &cyg::ssim_fwd, py::arg("y_true"), py::arg("y_pred"),
        py::arg("save_maps") = 0);
  m.def("ssim_bwd", &cyg::ssim_bwd, py::arg("x"), py::arg("y"), py::arg("am"),
        py::arg("bm"), py::arg("cm"), py::arg("dout"));
}
