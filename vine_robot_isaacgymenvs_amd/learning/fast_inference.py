"""The hand-written policy inference of one step (normalise -> MLP -> LSTM step, fp32 on the matrix cores for the default
network), shared by the trainer's rollout (``A2CAgent``) and the player's device path (``PpoPlayerContinuous``).

The methods read these attributes of the object they are mixed into: ``model``, ``device``, ``num_actors``, ``obs_shape``,
``rnn_states``, ``normalize_input``, ``fused_rollout``, ``rollout_lp16``, ``rollout_f32_terms``, ``_pending_fin`` (and, in
the low-precision rollout only, ``amp_dtype`` and ``optimizer``)."""
import torch

from . import fused


class FastInferenceMixin:
    def _setup_fast_inference(self):
        """Persistent buffers of the hand-written policy inference of the rollout (``_infer``):
        ``xh`` [N, XW + H] = [MLP output | normalised obs | pad | h] is the operand of ONE gate GEMM against
        ``wcat`` = [w_ih | 0 | w_hh]; operands are bfloat16 in the mixed-precision mode, fp32 otherwise."""
        net = self.model.a2c_network
        self._fast = None
        if not (self.fused_rollout and self.normalize_input and net.activation_is_elu and net.rnn_ln
                and net.rnn_units in (256, 512, 1024) and all(u % 4 == 0 for u in net.units)):
            return
        dev, N, H = self.device, self.num_actors, net.rnn_units
        op = self.amp_dtype if self.rollout_lp16 else torch.float32
        U, F_in = net.units[-1], self.obs_shape[0]
        width = U + (F_in if net.rnn_concat_input else 0)
        XW = (width + 15) // 16 * 16
        f = {"op": op, "U": U, "F": F_in, "XW": XW, "H": H,
             # two copies used alternately: the fused step kernel reads every column of its rows while other
             # workgroups write the new h block, so the h it produces goes to the OTHER buffer
             "xh2": [torch.zeros((N, XW + H), device=dev, dtype=op) for _ in range(2)], "cur": 0,
             "wcat": torch.zeros((4 * H, XW + H), device=dev, dtype=op),
             "acts": [torch.empty((N, u), device=dev, dtype=op) for u in net.units[:-1]],
             "y": torch.empty((N, H), device=dev), "h_tmp": torch.empty((N, H), device=dev),
             "c_tmp": torch.empty((N, H), device=dev)}
        f["x0_sep"] = None if net.rnn_concat_input else torch.empty((N, F_in), device=dev, dtype=op)
        f["ln_in_head"] = H == 256           # vine_policy_head applies the LayerNorm itself (one launch less per step)
        # padded layer-1 weight [units, 32] for the matrix-core kernel (mixed precision, concatenated input)
        f["w1p"] = None
        if (self.rollout_lp16 and net.rnn_concat_input and XW - U == 32
                and fused.linear_elu_mfma_ok(N, net.units[0], 32)):
            f["w1p"] = torch.zeros((net.units[0], 32), device=dev, dtype=op)
        # fp32 matrix-core kernels (vine_mlp3_elu_f32 / vine_lstm_step_f32): the default network at N % 512 == 0
        f["f32_mfma"] = (op == torch.float32 and net.rnn_concat_input and H == 256 and XW + H == 352
                         and XW - U == 32 and U == 64 and F_in <= 32 and tuple(net.units) == (256, 128, 64) and N % 512 == 0)
        f["f32_split"] = self.rollout_f32_terms if (f["f32_mfma"] and self.rollout_f32_terms in (6, 9)) else 0
        f["wt_f32"] = torch.empty(4 * H * (XW + H), device=dev) if (f["f32_mfma"] and not f["f32_split"]) else None
        # the three bf16 pieces of every recurrent weight, in the split step kernel's fragment order
        f["wt_split"] = (torch.empty(3 * 4 * H * (XW + H), device=dev, dtype=torch.bfloat16) if f["f32_split"] else None)
        f["w1p_f32"] = torch.zeros((net.units[0], 32), device=dev) if f["f32_mfma"] else None     # layer 1, zero-padded
        # the MLP's weights as fragments of bf16 pieces (vine_mlp3_elu_f32_split), rebuilt at every rollout start
        f["mlp_wt_split"] = (torch.empty(288 * 512, device=dev, dtype=torch.bfloat16)
                             if (f["f32_split"] and fused.MLP3_F32_SPLIT and N % 64 == 0) else None)
        f["bias_buf"] = torch.empty(4 * H, device=dev) if f["f32_mfma"] else None                  # b_ih + b_hh of a rollout
        self._fast = f

    def _infer_begin(self):
        """Once per rollout: operand copies of the recurrent weights and of h (the update changed the weights)."""
        f, net = self._fast, self.model.a2c_network
        r = net.rnn.rnn
        src = self.optimizer.shadow_of if self.rollout_lp16 else (lambda p: p)
        f["mlp"] = [(src(m.weight), m.bias) for m in net.actor_mlp if isinstance(m, torch.nn.Linear)]
        if f["f32_mfma"] and f["w1p"] is None and f.get("bias_buf") is not None:
            # fp32 rollout (the default): every operand copy of the rollout's start in ONE launch (round 4; they were nine:
            # profiles/r04/iteration_boundary_trace.txt) -- [w_ih | 0 | w_hh], the padded layer-1 weight, b_ih + b_hh, h into
            # the operand buffer, and the step-0 LSTM-state snapshots / slot-0 observation and done flags of the rollout
            cb = fused.CopyBatch()
            cb.add(cb.COPY, f["wcat"][:, :r.weight_ih_l0.shape[1]], r.weight_ih_l0)
            cb.add(cb.COPY, f["wcat"][:, f["XW"]:], r.weight_hh_l0)
            w1 = f["mlp"][0][0]
            cb.add(cb.COPY, f["w1p_f32"][:, :w1.shape[1]], w1)
            cb.add(cb.ADD, f["bias_buf"], r.bias_ih_l0, r.bias_hh_l0)
            f["bias"] = f["bias_buf"]
            f["cur"] = 0
            cb.add(cb.COPY, f["xh2"][0][:, f["XW"]:], self.rnn_states[0][0])
            for extra in getattr(self, "_rollout_start_copies", ()):
                cb.add(cb.COPY, *extra)
            self._rollout_start_copies = ()
            cb.flush(f["wcat"])
            st = torch.cuda.current_stream(self.device).cuda_stream
            if f["f32_split"]:
                fused._check(fused._lib().vine_lstm_tile_weights_split(
                    f["H"], f["XW"] + f["H"], f["wcat"].data_ptr(), f["wcat"].stride(0), f["wt_split"].data_ptr(), st),
                    "vine_lstm_tile_weights_split")
            else:
                fused._check(fused._lib().vine_lstm_tile_weights_f32(
                    f["H"], f["XW"] + f["H"], f["wcat"].data_ptr(), f["wcat"].stride(0), f["wt_f32"].data_ptr(), st),
                    "vine_lstm_tile_weights_f32")
            self._tile_mlp_weights(st)
            return
        f["wcat"][:, :r.weight_ih_l0.shape[1]].copy_(src(r.weight_ih_l0))
        f["wcat"][:, f["XW"]:].copy_(src(r.weight_hh_l0))
        # layer 1 through the matrix-core kernel too: operand = the obs block of xh plus the zero columns behind it
        if f["w1p"] is not None:                      # pad columns stay zero (allocated outside any capture)
            w1 = f["mlp"][0][0]
            f["w1p"][:, :w1.shape[1]].copy_(w1)
        f["bias"] = r.bias_ih_l0 + r.bias_hh_l0
        if f["f32_mfma"]:           # [w_ih | 0 | w_hh] in the step kernel's tile order; layer-1 weight padded to 32 columns
            w1 = f["mlp"][0][0]
            f["w1p_f32"][:, :w1.shape[1]].copy_(w1)
            st = torch.cuda.current_stream(self.device).cuda_stream
            if f["f32_split"]:
                fused._check(fused._lib().vine_lstm_tile_weights_split(
                    f["H"], f["XW"] + f["H"], f["wcat"].data_ptr(), f["wcat"].stride(0), f["wt_split"].data_ptr(), st),
                    "vine_lstm_tile_weights_split")
            else:
                fused._check(fused._lib().vine_lstm_tile_weights_f32(
                    f["H"], f["XW"] + f["H"], f["wcat"].data_ptr(), f["wcat"].stride(0), f["wt_f32"].data_ptr(), st),
                    "vine_lstm_tile_weights_f32")
            self._tile_mlp_weights(st)
        f["cur"] = 0
        f["xh2"][0][:, f["XW"]:].copy_(self.rnn_states[0][0])

    def _tile_mlp_weights(self, st):
        """The MLP weights in the split kernel's fragment order (once per rollout: the update changed them)."""
        f = self._fast
        if f.get("mlp_wt_split") is None or len(f["mlp"]) != 3:
            return
        (W1, _), (W2, _), (W3, _) = f["mlp"]
        fused._check(fused._lib().vine_mlp3_tile_weights_split(W1.data_ptr(), W1.stride(0), W1.shape[1], W2.data_ptr(),
                                                               W2.stride(0), W3.data_ptr(), W3.stride(0),
                                                               f["mlp_wt_split"].data_ptr(), st),
                     "vine_mlp3_tile_weights_split")

    def _infer(self, obs, commit=True):
        """Policy trunk for one step, no autograd: normalise -> [GEMM + bias/ELU kernel] x L -> ONE gate GEMM over
        [x | h] -> LSTM pointwise kernel (state updated in place) -> LayerNorm kernel.  ~10 launches.
        ``commit=False`` leaves the LSTM state untouched (the extra forward for the last values)."""
        lib = fused._lib()
        f, m = self._fast, self.model
        net, rms = m.a2c_network, m.running_mean_std
        N, H, XW = self.num_actors, f["H"], f["XW"]
        bf = int(f["op"] != torch.float32)
        st = torch.cuda.current_stream(self.device).cuda_stream
        xh, xh_next = f["xh2"][f["cur"]], f["xh2"][f["cur"] ^ 1]
        x0 = f["x0_sep"] if f["x0_sep"] is not None else xh[:, f["U"]:f["U"] + f["F"]]
        hp_ptr = (xh_next.data_ptr() + xh_next.element_size() * XW) if commit else None
        n_mlp = len(f["mlp"])
        mlp3 = (bf and f["w1p"] is not None and f["x0_sep"] is None and n_mlp == 3 and N % 64 == 0
                and f["U"] == 64 and f["F"] <= 32 and obs.is_contiguous() and obs.dtype == torch.float32
                and tuple(W.shape for W, _ in f["mlp"][1:]) == ((128, 256), (64, 128)) and f["mlp"][0][0].shape[0] == 256)
        f32k = bool(f["f32_mfma"]) and obs.is_contiguous() and obs.dtype == torch.float32 and n_mlp == 3
        if not f32k and getattr(self, "_pending_fin", None) is not None:
            # a deferred meter fold with no fp32 MLP launch to ride on (a caller changed the inference path between the
            # post-step kernel and this forward): run it as the one-workgroup launch it used to be -- never drop it
            fused._check(lib.vine_rollout_finalize(*self._pending_fin, st), "vine_rollout_finalize")
            self._pending_fin = None
        if f32k:
            # fp32 (the reference's rollout precision) on the matrix cores: normalisation + the three layers in one launch
            (W1, b1), (W2, b2), (W3, b3) = f["mlp"]
            fin = getattr(self, "_pending_fin", None)      # the previous step's meter fold rides on workgroup 0 (round 4)
            self._pending_fin = None
            if f.get("mlp_wt_split") is not None:
                # exact products from bf16 pieces, as the LSTM step below (four waves share the rows, split the units)
                fused._check(lib.vine_mlp3_elu_f32_split(N, xh.data_ptr(), xh.stride(0), obs.data_ptr(), f["F"],
                                                         rms.running_mean.data_ptr(), rms.running_var.data_ptr(),
                                                         float(rms.epsilon), 5.0, f["mlp_wt_split"].data_ptr(),
                                                         b1.data_ptr(), b2.data_ptr(), b3.data_ptr(), 1.0,
                                                         f["f32_split"] | (fused.MLP3_F32_SPLIT_RT << 8) | (int(fused.ROLLOUT_F32_DUAL) << 16),
                                                         *(fin if fin is not None else (None, 0.0, None, None, 0)), st),
                             "vine_mlp3_elu_f32_split")
            else:
                fused._check(lib.vine_mlp3_elu_f32_fin(N, xh.data_ptr(), xh.stride(0), obs.data_ptr(), f["F"],
                                                       rms.running_mean.data_ptr(), rms.running_var.data_ptr(),
                                                       float(rms.epsilon), 5.0, f["w1p_f32"].data_ptr(), 32, b1.data_ptr(),
                                                       256, W2.data_ptr(), W2.stride(0), b2.data_ptr(), 128, W3.data_ptr(),
                                                       W3.stride(0), b3.data_ptr(), 64, 1.0,
                                                       *(fin if fin is not None else (None, 0.0, None, None, 0)), st),
                             "vine_mlp3_elu_f32_fin")
        elif mlp3:
            # observation normalisation and the whole MLP in ONE launch: the kernel normalises the raw observations
            # itself, writes them (bf16, zero-padded) into the LSTM operand's observation block and carries the
            # activations through the three layers in registers (the intermediate activations are not needed here)
            (W1, b1), (W2, b2), (W3, b3) = f["mlp"]
            fused._check(lib.vine_mlp3_elu_mfma(N, xh.data_ptr() + 2 * f["U"], xh.stride(0), obs.data_ptr(), f["F"],
                                                rms.running_mean.data_ptr(), rms.running_var.data_ptr(),
                                                float(rms.epsilon), 5.0, f["w1p"].data_ptr(), b1.data_ptr(), 256,
                                                W2.data_ptr(), W2.stride(0), b2.data_ptr(), 128, W3.data_ptr(), W3.stride(0),
                                                b3.data_ptr(), 64, 1.0, None, None, xh.data_ptr(), xh.stride(0), st),
                         "vine_mlp3_elu_mfma")
        elif not f32k:
            fused._check(lib.vine_normalize_obs(N, f["F"], obs.data_ptr(), rms.running_mean.data_ptr(),
                                                rms.running_var.data_ptr(), float(rms.epsilon), 5.0, x0.data_ptr(),
                                                x0.stride(0), bf, st), "vine_normalize_obs")
        x = x0
        for i, (W, b) in enumerate(f["mlp"] if not (mlp3 or f32k) else ()):
            out = xh if i == n_mlp - 1 else f["acts"][i]
            if i == 0 and f["w1p"] is not None:
                fused._check(lib.vine_linear_elu_mfma(N, W.shape[0], 32, xh.data_ptr() + 2 * f["U"], xh.stride(0),
                                                      f["w1p"].data_ptr(), 32, b.data_ptr(), 1.0, out.data_ptr(),
                                                      out.stride(0), st), "vine_linear_elu_mfma")
            elif bf and fused.linear_elu_mfma_ok(N, W.shape[0], W.shape[1]):
                fused._check(lib.vine_linear_elu_mfma(N, W.shape[0], W.shape[1], x.data_ptr(), x.stride(0), W.data_ptr(),
                                                      W.stride(0), b.data_ptr(), 1.0, out.data_ptr(), out.stride(0), st),
                             "vine_linear_elu_mfma")
            else:
                z = fused._mm(x, W.t())
                fused._check(lib.vine_bias_elu(N, z.shape[1], z.data_ptr(), b.data_ptr(), 1.0, out.data_ptr(),
                                               out.stride(0), bf, st), "vine_bias_elu")
            x = out
        h32, c = self.rnn_states[0][0], self.rnn_states[1][0]
        h_out, c_out = (h32, c) if commit else (f["h_tmp"], f["c_tmp"])
        Kx = XW + H
        if f32k and f["f32_split"]:
            # gate GEMM over [x | h] + the cell update: fp32 operands, every product exact from bf16 pieces (9 pairs)
            fused._check(lib.vine_lstm_step_f32_split(N, H, Kx, xh.data_ptr(), xh.stride(0), f["wt_split"].data_ptr(),
                                                      f["bias"].data_ptr(), c.data_ptr(), h_out.data_ptr(), H,
                                                      c_out.data_ptr(), hp_ptr, xh_next.stride(0),
                                                      f["f32_split"] | (int(fused.rollout_f32_nsplit(N)) << 16), st),
                         "vine_lstm_step_f32_split")
            gates = None
        elif f32k:
            # gate GEMM over [x | h] + the cell update, fp32 on the matrix cores
            fused._check(lib.vine_lstm_step_f32(N, H, Kx, xh.data_ptr(), xh.stride(0), f["wt_f32"].data_ptr(),
                                                f["bias"].data_ptr(), c.data_ptr(), h_out.data_ptr(), H, c_out.data_ptr(),
                                                hp_ptr, xh_next.stride(0), st), "vine_lstm_step_f32")
            gates = None
        elif bf and N % 64 == 0 and Kx in (128, 256, 288, 320, 352, 384, 512) and H % 16 == 0:
            # gate GEMM over [x | h] fused with the pointwise update on the matrix cores
            fused._check(lib.vine_lstm_step_mfma(
                N, H, Kx, xh.data_ptr(), xh.stride(0), None, 0, 0, f["wcat"].data_ptr(), f["wcat"].stride(0), None, 4 * H,
                f["bias"].data_ptr(), c.data_ptr(), None, 0, h_out.data_ptr(), H, c_out.data_ptr(), None,
                hp_ptr, None, 0, Kx, st), "vine_lstm_step_mfma")
            gates = None
        else:
            gates = fused._mm(xh, f["wcat"].t())
        if gates is not None:
            fused._check(lib.vine_lstm_cell_forward(
                N, H, gates.data_ptr(), 4 * H, None, f["bias"].data_ptr(), c.data_ptr(), None, 0, h_out.data_ptr(), H,
                c_out.data_ptr(), None, hp_ptr, None, 0, bf, XW + H, st), "vine_lstm_cell_forward")
        if commit:
            f["cur"] ^= 1
        if f["ln_in_head"]:              # the policy-head kernel normalises (reads the state before rollout_post clears it)
            return h_out
        y = f["y"]
        fused._check(lib.vine_layernorm_forward(N, H, h_out.data_ptr(), net.layer_norm.weight.data_ptr(),
                                                net.layer_norm.bias.data_ptr(), float(net.layer_norm.eps), y.data_ptr(),
                                                None, None, st), "vine_layernorm_forward")
        return y

    # ---- the policy head inside the step launch (vine_step_rollout / vine_step_eval): its operands, marshalled once
    def _head_prep(self, hw, hc):
        """``hw`` [3, 256] = gamma_u w_k[u] and ``hc`` [3] = beta . w_k + b_k for k = mu_0, mu_1, value: the LayerNorm folded
        into the head's rows (once per rollout / evaluation run: the update changed the weights)."""
        net = self.model.a2c_network
        st = torch.cuda.current_stream(self.device).cuda_stream
        fused._check(fused._lib().vine_rollout_head_prep(net.layer_norm.weight.data_ptr(), net.layer_norm.bias.data_ptr(),
                                                         net.mu.weight.data_ptr(), net.mu.bias.data_ptr(),
                                                         net.value.weight.data_ptr(), net.value.bias.data_ptr(),
                                                         hw.data_ptr(), hc.data_ptr(), st), "vine_rollout_head_prep")

    def _h_op_next(self):
        """Address of the operand copy of h that the NEXT step reads (in the buffer ``_infer`` just switched to): what a
        kernel that clears the LSTM state of finished envs has to clear with it."""
        f = self._fast
        xh = f["xh2"][f["cur"]]
        return xh.data_ptr() + xh.element_size() * f["XW"]

    def _fill_head_args(self, args, y, hw, hc):
        """The fields that ``abi.RolloutArgs`` and ``abi.EvalArgs`` share: the LSTM output rows ``y`` of this step, the
        head's operands, and the LSTM-state rows that the step clears for finished envs."""
        f, net = self._fast, self.model.a2c_network
        args.y, args.hw, args.hc, args.logstd = y.data_ptr(), hw.data_ptr(), hc.data_ptr(), net.sigma.data_ptr()
        args.ln_eps = float(net.layer_norm.eps)
        args.h_state, args.c_state = self.rnn_states[0].data_ptr(), self.rnn_states[1].data_ptr()
        args.h_op, args.h_op_stride = self._h_op_next(), f["XW"] + f["H"]
