/*
 * fa.h -- C ABI of the MI355X FedAvg aggregation path (libfa.so).
 *
 * The reference has no plugin/FFI seam: the reduction is inline in the
 * aggregator's main() (pipeline_simulation/aggregator.cpp:55-167).  These
 * entry points replace that inline code; each declaration names the reference
 * lines it stands in for.  Plain pointers and sizes only, no torch types, no
 * C++ exceptions across the boundary.  Every call returns FA_OK (0) or a
 * negative fa_status; fa_last_error() gives a thread-local message.
 *
 * Threading: one fa_ctx per aggregator; calls on one ctx are serialized by the
 * caller (the reference's single consumer main thread, aggregator.cpp:60/:113).
 * Device work runs on ctx-owned HIP streams (one compute + one copy stream per
 * GPU, plus a high-priority exchange stream per GPU for FA_SHARD_CLIENT_RS only)
 * or on the caller's stream for fa_reduce_device.
 *
 * Numerics (tests/, DESIGN.md "Parity"):
 *   FA_FEDAVG  out_i = sum_k w_k x_{k,i} as an ordered fp32 FMA chain in client
 *              order starting from +0 (== libtorch acc.add_(x_k, w_k)),
 *              bf16 and fp16 inputs widened exactly (fp16 subnormals
 *              included), a bf16 or fp16 output rounded to nearest-even once
 *              at the end.  Bit-exact vs oracle/ on every GPU layout
 *              except FA_SHARD_CLIENT_RS (summation order changes, <=1e-6
 *              relative to sum_k |w_k x_k|).
 *   FA_LITERAL out_i = fl(fl(x_i + x_i) / divisor), x = the LAST client
 *              submitted (aggregator.cpp:63-88 with parts/parts_ aliased,
 *              systemAPI.cpp:34-37); divisor defaults to kTrainSize_10 = 1000
 *              (aggregator.cpp:48).  Correctly rounded division.  A 16-bit
 *              output is fl16(fl32(fl32(x + x) / divisor)).
 *   FA_TRIMMED coordinate-wise trimmed mean over the D clients, specified bit for bit.  For every
 *              element i, with trim t (0 <= t, 2t < D):
 *              1. x_{k,i} is widened to fp32 exactly (bf16, fp16 with its subnormals).
 *              2. The D values are sorted ascending under this total order: any NaN (either sign) is
 *                 greater than +inf; otherwise numeric order; -0 < +0; equal bit patterns are
 *                 interchangeable.  It is the order of the unsigned key k(x) = 0xFFFFFFFF if x is NaN,
 *                 ~bits if the sign bit is set, bits | 0x80000000 otherwise.  A sorted NaN decodes to
 *                 some quiet NaN (payload unspecified).
 *              3. acc = +0, then acc = fl32(acc + s_j) for j = t .. D-t-1 in ascending order (plain adds).
 *              4. out_i = fl32(acc / (float)(D - 2t)), correctly rounded division (as FA_LITERAL).
 *              5. A bf16 or fp16 output is that rounded once to nearest-even, as for FA_FEDAVG.
 *              Weights are ignored (as for FA_LITERAL).  Up to t NaN or +inf values per element are
 *              trimmed away at the top and t values of -inf at the bottom.  t = 0 is an unweighted
 *              mean summed in ascending order (not the FedAvg chain); t = (D-1)/2 is the median (the
 *              middle value for odd D, fl(fl(a+b)/2) of the two middle values for even D); D = 1 is
 *              fl(fl(+0 + x)/1).  D <= FA_TRIMMED_MAX_CLIENTS: the sort runs on one GPU in
 *              one pass.  Added without a new FA_ABI_VERSION: fa_trimmed_device(NULL, 0, ptrs, D, 0, ...)
 *              touches no device and answers FA_OK -- that is how a caller probes for it.
 *   Server optimizer (fa_set_server_opt, fa_server_opt_device): an element-wise update rule applied to the
 *              round's aggregate (Reddi et al., "Adaptive Federated Optimization", Algorithm 2: FedAvgM,
 *              FedAdagrad, FedAdam, FedYogi), specified bit for bit.  Per element, a is the part's fp32
 *              aggregate: the ordered FMA chain for FA_FEDAVG, step 4 of the rule above for FA_TRIMMED, in
 *              both cases before any rounding to a 16-bit output.  The state is x (the global model, an
 *              fp32 master also for bf16 / fp16 buckets), m and v, all fp32, kept on the GPU across rounds.
 *              The parameters are the floats lr, beta1, beta2, tau; on the host, in fp32,
 *              c1 = fl(1 - beta1), c2 = fl(1 - beta2).  Every operation below is one IEEE fp32 operation
 *              rounded to nearest-even; there is no fused multiply-add anywhere in the stage; division and
 *              square root are correctly rounded; subnormals are kept.
 *                d  = fl(a - x)
 *                FA_OPT_MOMENTUM (FedAvgM):  m' = fl(fl(beta1 m) + d);  x' = fl(x + fl(lr m'));
 *                                            v is not read, written or allocated
 *                FA_OPT_ADAGRAD / ADAM / YOGI:  m' = fl(fl(beta1 m) + fl(c1 d));  q = fl(d d)
 *                  ADAGRAD: v' = fl(v + q)
 *                  ADAM:    v' = fl(fl(beta2 v) + fl(c2 q))
 *                  YOGI:    u = fl(c2 q); s = fl(v - q);
 *                           v' = fl(v - u) if s > 0, fl(v + u) if s < 0, v if s == 0, a quiet NaN if s is NaN
 *                  x' = fl(x + fl(fl(lr m') / fl(fl(sqrt(v')) + tau)))
 *                out = x' (a bf16 / fp16 output: x' rounded once to nearest-even, as for FA_FEDAVG)
 *              No bias correction, as in the paper.  NaN and inf propagate (NaN payloads unspecified);
 *              robustness comes from combining the stage with FA_TRIMMED.
 *              Bootstrap: the first reduction of a part that has no master (none was set with
 *              fa_server_opt_set_state and none was stepped yet) does x' = a, m' = +0, v' = +0, out = a
 *              rounded to the out dtype; `steps` stays 0.  Every later reduction is one step and adds 1 to
 *              `steps`.  Added without a new FA_ABI_VERSION: fa_server_opt_device with n == 0 touches no
 *              device and answers FA_OK -- that is how a caller probes for it.
 *   Clip stage (fa_set_clip): per-client L2 norm clipping of the updates of an FA_FEDAVG part (norm-bounded
 *              FedAvg: Sun et al., "Can You Really Backdoor Federated Learning?"; the deterministic half of
 *              DP-FedAvg).  Part-level state: g, an fp32 "reference" of n elements -- the global model the
 *              owners last received -- and whether it exists.  Per round, with weights w_k and the fp32
 *              C = max_norm > 0:
 *              1. Squared distance.  For every client k: x_{k,i} is widened to fp32 exactly,
 *                 d = fl32(x_{k,i} - g_i), q = (double)d * (double)d (exact in fp64), Q_k = sum_i q.  The
 *                 summation order is NOT specified: every partial sum is an fp64 add of non-negative terms, so
 *                 whatever the order |Q_k - exact| <= n * 2^-53 * exact.  No floating-point atomics: for one
 *                 layout (GPU count, tuning, n, D) the result is the same bits on every run.  On range shards
 *                 and range pieces the per-shard / per-piece sums are added on the host in fp64, in GPU order
 *                 and then piece order.
 *              2. Scale (fa_clip_scale, pure host arithmetic).  N = sqrt(Q_k) in fp64, correctly rounded.  If N
 *                 is NaN or +inf, client k is EXCLUDED this round; else if N <= (double)C, s_k = 1.0f; else
 *                 s_k = (float)((double)C / N).
 *              3. Weights.  w'_k = fl32(w_k * s_k) for the included clients.  In fp64, in client order,
 *                 W = the sum over all D of (double)w_k and W' = the sum over the included clients of
 *                 (double)w'_k; c0 = (float)(W - W').
 *              4. Aggregate.  acc = +0; if c0 != 0, acc = fmaf(c0, g_i, acc); then acc = fmaf(w'_k, x_{k,i}, acc)
 *                 for the included k in ascending order: the FA_FEDAVG chain with g as an extra first term,
 *                 since sum_k w_k s_k (x_k - g) + W g = sum_k (w_k s_k) x_k + (W - sum_k w_k s_k) g.  The mass
 *                 taken from clipped or excluded owners stays on the reference.  If no owner is clipped or
 *                 excluded, c0 == 0 and the result is bit for bit the plain FA_FEDAVG aggregate.  With zero
 *                 included clients the aggregate is that first term alone (+0 when c0 == 0).
 *              5. The aggregate is the part's fp32 aggregate a: it feeds the server-optimizer stage if the part
 *                 has one, otherwise it is rounded once to the out dtype as for FA_FEDAVG.
 *              6. Reference update.  After the round g becomes the part's output widened to fp32 (for a 16-bit
 *                 out dtype the rounded values): exactly what the owners receive, with or without a server
 *                 optimizer.
 *              7. Bootstrap.  A round on a part that has no reference does no clipping: the plain aggregate,
 *                 all s_k = 1, nothing excluded, Q_k reported as 0.  The reference is then set from its output.
 *              A reducing call of such a part enqueues the norm pass on every GPU, waits for the D sums (one
 *              stream round trip more than a plain round) and then enqueues the chain.  Added without a new
 *              FA_ABI_VERSION: fa_clip_sumsq_device with n == 0 touches no device and answers FA_OK -- that is
 *              how a caller probes for it.
 *   Krum stage (fa_set_krum): distance-based selection of the owners of an FA_FEDAVG part (Krum / Multi-Krum:
 *              Blanchard et al., "Machine Learning with Adversaries: Byzantine Tolerant Gradient Descent", NeurIPS
 *              2017).  The owners whose whole bucket lies far from everyone else's are left out, the rest are
 *              averaged with their own weights.  No part-level state and no reference model.  Parameters: f, the
 *              number of owners assumed Byzantine, and m, how many owners to keep, with 0 <= f, 2 f + 2 < D (so
 *              D >= 3), 1 <= m <= D - f and D <= FA_KRUM_MAX_CLIENTS; m = 1 is Krum, m = D - f the usual
 *              Multi-Krum.  Per round, with weights w_k:
 *              1. Distances.  For every unordered pair a < b: x is widened to fp32 exactly,
 *                 d = fl32(x_{a,i} - x_{b,i}), q = (double)d * (double)d (exact in fp64), Q_ab = sum_i q.  As in
 *                 the clip stage the summation order is NOT specified: every partial sum is an fp64 add of
 *                 non-negative terms, so whatever the order |Q_ab - exact| <= n * 2^-53 * exact.  No floating-point
 *                 atomics: for one layout (GPU count, tuning, n, D) the result is the same bits on every run.  Each
 *                 pair is computed once and mirrored: the reported D x D matrix is bit-symmetric.  Its diagonal is
 *                 +0 by definition -- it is not computed, also for a bucket that holds a NaN.  NaN and inf
 *                 propagate into Q.  On range shards and range pieces the per-shard / per-piece matrices are added
 *                 on the host in fp64, in GPU order and then piece order.
 *              2. Scores (fa_krum_select, pure host arithmetic in fp64).  For client k take the D - 1 values Q_kj,
 *                 j != k, replace NaN by +inf and sort them ascending; S_k = the first D - f - 2 of them added in
 *                 ascending order, starting from +0.
 *              3. Selection.  Order the clients by (S_k, k) ascending: ties go to the lower index.  The selected
 *                 set is the first m of them, except that a client with S_k = +inf is never selected: fewer than m
 *                 may be selected, possibly none.
 *              4. Weights (fa_krum_weights, pure host arithmetic).  In fp64, in client order, W = the sum of
 *                 (double)w_k over all D clients and W_s = the same sum over the selected ones.  If all D are
 *                 selected, or W_s is not > 0, or W / W_s is not finite: w'_k = w_k.  Otherwise
 *                 w'_k = (float)((double)w_k * (W / W_s)).  The round keeps its total mass: for m = 1 the result is
 *                 the chosen owner's bucket times about W (each element fl32(w'_k x)), not a bit copy of it.
 *              5. Aggregate.  The FA_FEDAVG chain from +0 over the selected clients in ascending client order with
 *                 the weights w'.  With nobody deselected it is the plain FA_FEDAVG aggregate bit for bit; with
 *                 nobody selected it is +0.  It is the part's fp32 aggregate a: it feeds the server-optimizer
 *                 stage if the part has one, otherwise it is rounded once to the out dtype as for FA_FEDAVG.
 *              A reducing call of such a part enqueues the distance pass on every GPU, waits for the matrices (one
 *              stream round trip more than a plain round), selects on the host and then enqueues the chain.  Added
 *              without a new FA_ABI_VERSION: fa_pairdist_device with n == 0 touches no device, writes D * D zeros
 *              and answers FA_OK -- that is how a caller probes for it.
 *   Bulyan stage (fa_set_bulyan): iterated Krum, then a median-centred mean, on an FA_TRIMMED part (El Mhamdi,
 *              Guerraoui, Rouault, "The Hidden Vulnerability of Distributed Learning in Byzantium", ICML 2018).  Krum
 *              alone lets one coordinate of a selected owner be arbitrarily wrong; a trimmed mean alone ignores how
 *              far an owner's whole bucket lies from the others; Bulyan first picks theta = D - 2f owners by running
 *              Krum repeatedly and then, per element, averages the theta - 2f picked values closest to their median.
 *              Parameter: f, the number of owners assumed Byzantine, 0 <= f and 4 f + 3 <= D <=
 *              FA_TRIMMED_MAX_CLIENTS.  Weights are ignored, as for FA_TRIMMED; the part's trim is not used while the
 *              stage is set; no state across rounds.  Per round:
 *              1. Distances.  Exactly rule 1 of the Krum stage: the D x D matrix Q, bit-symmetric, +0 diagonal, the
 *                 order of the fp64 sums free within n 2^-53 relative, no atomics; shards and pieces are added on the
 *                 host in GPU order, then piece order.
 *              2. Iterated selection (fa_bulyan_select, pure host arithmetic in fp64).  R = all D clients in ascending
 *                 order, theta = D - 2f.  Until theta clients are picked: c = max(1, |R| - f - 2) (the paper leaves
 *                 the count open once |R| < 2f + 3; this is the choice made here); for every k in R take Q_kj for j in
 *                 R, j != k, replace NaN by +inf and sort ascending; S_k = the first min(c, |R| - 1) of them added in
 *                 ascending order from +0, each add one rounded fp64 add (a lone remaining client scores +0); the pick
 *                 is the smallest (S_k, k).  If its S is +inf the selection stops and fewer than theta are picked;
 *                 otherwise it is appended to the pick order and removed from R.
 *              3. Centred mean.  theta' = the number picked.  If theta' = 0 the aggregate is +0.  Otherwise
 *                 keep = max(1, theta' - 2f) and every element is the centred mean of rule 4 over the picked clients'
 *                 values (they are passed in ascending client order; the order does not matter to the result).
 *              4. Centred mean of theta values keeping `keep` (1 <= keep <= theta), per element.  Widen to fp32 and
 *                 sort ascending under the FA_TRIMMED total order (the same keys) into s_0 .. s_{theta-1}.
 *                 c_lo = s_{(theta-1)/2}, c_hi = s_{theta/2} (integer division; for odd theta both are the median).
 *                 j = 0; while j < theta - keep: d_hi = fl32(s_{j+keep} - c_hi), d_lo = fl32(c_lo - s_j); if
 *                 d_hi < d_lo then j = j + 1, otherwise stop (an IEEE comparison, false when either side is NaN;
 *                 subnormal differences are kept).  acc = +0, then acc = fl32(acc + s_u) for u = j .. j + keep - 1
 *                 ascending; out = fl32(acc / (float)keep), correctly rounded; a 16-bit output is that rounded once,
 *                 as for FA_TRIMMED.  keep == theta is FA_TRIMMED with trim 0 bit for bit.  Ties keep the lower
 *                 window; a NaN above the window is never slid into; a -inf at the bottom is slid away whenever the
 *                 centre is finite.  On finite data without ties the window holds exactly the `keep` values nearest
 *                 the median.
 *              5. Place in the round.  The value of rule 3 is the part's fp32 aggregate a, exactly where step 4 of
 *                 FA_TRIMMED is: it feeds the noise stage and the server optimizer if present, otherwise it is rounded
 *                 once to the out dtype.  A reducing call does the distance pass, one host wait, the selection and
 *                 then the launches, as a Krum part does.
 *              Added without a new FA_ABI_VERSION: fa_centered_device with n == 0 touches no device and answers
 *              FA_OK -- that is how a caller probes for it.
 *   Geomed stage (fa_set_geomed): the geometric median of the owners of an FA_FEDAVG part by smoothed Weiszfeld
 *              iterations (Pillutla, Kakade, Harchaoui, "Robust Aggregation for Federated Learning", IEEE TSP 2022,
 *              "RFA").  It keeps the owners' weights, needs no f and no reference model, has breakdown point 1/2 and
 *              discards nobody: an owner far from the others is down-weighted, not dropped.  Parameters: iters = T, 1 <=
 *              T <= FA_GEOMED_MAX_ITERS, and nu, an fp32 value that is finite and > 0: the smoothing floor on a
 *              distance.  D <= FA_GEOMED_MAX_CLIENTS.  No state across rounds.  Per round, with weights w_k:
 *              0. Start.  A client whose w_k is not > 0 (zero, negative or NaN) is excluded for the round.  W = the
 *                 fp64 sum of (double)w_k over the remaining clients, in client order; alpha^0_k = w_k.
 *              1. Pass t (t = 0 .. T-1), over the currently included clients in ascending client order.  Per element
 *                 v^t_i is the FA_FEDAVG chain, acc = +0; acc = fmaf(alpha^t_k, x_{k,i}, acc), inputs widened exactly:
 *                 bit for bit what fa_reduce_device gives for those clients and weights into an f32 output.  For
 *                 every included k: d = fl32(x_{k,i} - v^t_i), q = (double)d * (double)d, Q^t_k = sum_i q; as in the
 *                 clip stage the order of the fp64 adds is free within n 2^-53 relative, there are no floating-point
 *                 atomics and one layout gives the same bits on every run.  For every included k: B_k = the exact
 *                 count of elements of bucket k that are NaN or +-inf after widening.  One fused kernel does all
 *                 three: the buckets are read once and v is not stored.  On range shards and range pieces Q and B are
 *                 added on the host in fp64, in GPU order and then piece order.
 *              2. Non-finite buckets.  After a pass every included client with B_k > 0 is excluded for the rest of the
 *                 round.  If that removed anyone the pass's v was poisoned and its distances are void: alpha^t is
 *                 recomputed by rule 4 over the remaining clients (for t = 0 from w, otherwise from the last valid Q)
 *                 and the pass is repeated.  Buckets do not change within a round, so this happens at most once, and
 *                 only at t = 0.
 *              3. Distances.  N_k = sqrt(Q^t_k) in fp64.  A client whose N_k is NaN or +inf (an fp32 overflow in d or
 *                 in v) is excluded from now on; the pass is not repeated.
 *              4. Weights (fa_geomed_weights, pure host arithmetic in fp64).  For included k:
 *                 beta_k = (double)w_k / max((double)nu, N_k); B = the sum of beta_k in client order.  If B is not > 0,
 *                 or W / B is not finite: alpha^{t+1}_k = w_k.  Otherwise alpha^{t+1}_k = (float)(beta_k * (W / B)).
 *                 The round keeps the mass W of the owners that entered it (the Krum stage's convention).
 *              5. Aggregate.  After pass T-1 and rules 3-4 the aggregate is the plain FA_FEDAVG chain from +0 over the
 *                 included clients in ascending client order with the weights alpha^T; with nobody included it is +0.
 *                 It is the part's fp32 aggregate a: it feeds the noise stage and the server optimizer if the part
 *                 has them, otherwise it is rounded once to the out dtype as for FA_FEDAVG.
 *              6. Costs.  A reducing call makes T host round trips (T + 1 on a round with a non-finite bucket), then
 *                 enqueues the final chain without waiting: T fused passes plus one ordinary chain, T + 1 reads of the
 *                 data.
 *              Added without a new FA_ABI_VERSION: fa_geomed_pass_device with n == 0 touches no device, writes zeros
 *              and answers FA_OK -- that is how a caller probes for it.
 *   Noise stage (fa_set_noise, fa_noise_device, fa_noise_host): Gaussian noise on the round's aggregate, the other
 *              half of DP-FedAvg (McMahan et al., "Learning Differentially Private Recurrent Language Models"):
 *              a'_i = a_i + stddev z_i with z_i a standard normal, specified bit for bit.  Parameters: stddev
 *              (fp32, finite, > 0), seed (u64), stream (u32; within the library the part id) and round (u32).
 *              Element i is the element's index in the whole bucket, never the index within a shard or a piece:
 *              the result does not depend on the layout (GPU count, shards, pieces, pointer phase).  Every step
 *              of rules 2-4 is one IEEE fp32 operation rounded to nearest-even; nothing is fused; division and
 *              square root are correctly rounded; subnormals are kept.
 *              1. Generator.  Philox4x32-10 (Salmon et al., "Parallel Random Numbers: As Easy as 1, 2, 3", SC'11):
 *                 multipliers 0xD2511F53 and 0xCD9E8D57, key increments 0x9E3779B9 and 0xBB67AE85, ten rounds.  For
 *                 group j = i >> 2: counter = (lo32(j), hi32(j), round, stream), key = (lo32(seed), hi32(seed)).
 *                 Of the output words (r0, r1, r2, r3) the pair (r0, r1) makes the normals of elements 4j and
 *                 4j + 1, the pair (r2, r3) those of 4j + 2 and 4j + 3; in a pair the first word gives the radius
 *                 (rule 2), the second the direction (rule 3).  Known answers (counter; key; output):
 *                   0 0 0 0; 0 0; 6627e8d5 e169c58d bc57ac4c 9b00dbd8
 *                   ffffffff x 4; ffffffff x 2; 408f276d 41c83b0e a20bc7c6 6d5451fd
 *                   243f6a88 85a308d3 13198a2e 03707344; a4093822 299f31d0; d16cfe09 94fdcceb 5001e420 24126ea1
 *              2. Radius, from a word r.  N = r + 1 as an integer in 1 .. 2^32, b the position of its leading one,
 *                 mant = the top 24 bits of N (bit b moved to bit 23, lower bits truncated, a short N shifted up).
 *                 m = (float)mant * 2^-23 in [1, 2), e = b - 32: u = m 2^e lies in (0, 1].  If m > fl(sqrt 2):
 *                 m = fl(m * 0.5f) (exact), e = e + 1.  f = fl(m - 1); s = fl(f / fl(2 + f)); t = fl(s s);
 *                   p = fl(C9 t); p = fl(p + C7); p = fl(p t); p = fl(p + C5); p = fl(p t); p = fl(p + C3);
 *                   p = fl(p t); p = fl(p s); p = fl(p + s); l = fl(p + p),       Ck = fl(1/k)
 *                 L = fl(fl((float)e * LN2) + l), LN2 = fl(ln 2) = 0x1.62e43p-1; R = sqrt(fl(-2 * L)).
 *                 r = 0xFFFFFFFF gives R = -0 (both normals are zeros); the largest R, from r = 0, is 6.6604.
 *              3. Direction, from a word r.  q = r >> 30; k = (r & 0x3FFFFFFF) >> 6;
 *                 v = (float)(k - 2^23) * 2^-23 in [-1, 1); x = fl(v * PI4), PI4 = fl(pi/4) = 0x1.921fb6p-1;
 *                 y = fl(x x);
 *                   p = fl(S9 y); p = fl(p + S7); p = fl(p y); p = fl(p + S5); p = fl(p y); p = fl(p + S3);
 *                   p = fl(p y); p = fl(p x); sx = fl(p + x),    S3 = fl(-1/6), S5 = fl(1/120), S7 = fl(-1/5040),
 *                                                                 S9 = fl(1/362880)
 *                   p = fl(K8 y); p = fl(p + K6); p = fl(p y); p = fl(p + K4); p = fl(p y); p = fl(p + K2);
 *                   p = fl(p y); cx = fl(p + 1),                 K2 = fl(-1/2), K4 = fl(1/24), K6 = fl(-1/720),
 *                                                                 K8 = fl(1/40320)
 *                 The angle is q pi/2 + x: (cos, sin) = (cx, sx) for q = 0, (-sx, cx) for 1, (-cx, -sx) for 2,
 *                 (sx, -cx) for 3.  The four quadrants of [-pi/4, pi/4) tile the circle; no rotation by pi/4 is
 *                 applied, so a small component keeps the relative accuracy of sx.
 *              4. Normals and output.  From one word pair z0 = fl(R cos), z1 = fl(R sin);
 *                 a'_i = fl(a_i + fl(stddev z_i)).  A NaN or inf in a propagates (NaN payloads unspecified).
 *              5. Place in the round.  a is the part's fp32 aggregate exactly as for the server optimizer (the
 *                 plain chain, the clipped or Krum subset chain, step 4 of FA_TRIMMED, rule 3 of the Bulyan stage); a'
 *                 takes its place: it
 *                 feeds the server-optimizer stage if there is one, otherwise it is rounded once to the out dtype.
 *                 The clip stage's new reference is the output as before: what the owners receive, noise included.
 *                 A clip bootstrap round (no reference, nothing clipped) still gets its noise; that it bounds
 *                 nothing is the caller's business.  One reducing call uses the part's current round and then adds
 *                 1 to it; the call that would use 2^32 fails with FA_ERR_STATE.
 *              Accuracy: against the same transform in fp64 from the same u and angle every normal lies within
 *              8 * 2^-24 * max(1, |z|) (measured: 4.1 of these units).  Limits: 24-bit uniforms, so |z| <= 6.6604
 *              and the tails end there; fp32 arithmetic, as in the usual DP libraries; Philox is not a
 *              cryptographic generator: the privacy of the result rests on the seed staying secret and on a
 *              (seed, stream, round) triple never being used twice.  Added without a new FA_ABI_VERSION:
 *              fa_noise_device with n == 0 touches no device and answers FA_OK -- that is how a caller probes for it.
 *   MX8 receipts (fa_set_mx8, fa_submit_mx8, fa_mx8_expand_device, fa_mx8_encode, fa_mx8_decode): a client sends
 *              its update x_k - g against the model g it was last sent, as 8-bit integers with one power-of-two
 *              scale per 32 elements (the MXINT8 layout): 33 bytes per 32 elements where fp32 takes 128.  The
 *              compressed bytes cross the wire and PCIe; a kernel rebuilds the ordinary slot x = g + d, and
 *              everything downstream (every mode, stage, layout) sees an ordinary receipt.
 *              Format.  A compressed bucket of n elements is two arrays: q, n bytes, q_i an int8 in two's
 *              complement, all 256 codes valid; e, ceil(n / 32) bytes, e_b the scale of block b = elements
 *              [32 b, 32 b + 32).  The block of element i is i >> 5 with i the element's index in the whole
 *              bucket, never the index within a shard or a piece.
 *              Decode (fa_mx8_decode; the kernel does the same steps):
 *              1. If E = e_b is 255, every d_i of the block is a quiet NaN (payload unspecified).
 *              2. Otherwise s = 2^(E - 133) and d_i = fl32((float)q_i * s), one IEEE fp32 multiply.  s is an fp32
 *                 value for every E in 0 .. 254, subnormal below E = 7; subnormals are kept.  The product is exact
 *                 for every (q, E) but one: q = -128 at E = 254 is -2^128 and rounds to -inf.
 *              3. Expansion into a slot of dtype `in` against a reference of dtype `ref`:
 *                 x_i = fl32(widen(g_i) + d_i), one rounding, g widened exactly (bf16; fp16 with its subnormals).  A
 *                 16-bit slot stores x_i rounded once more to nearest-even, as every 16-bit output here.  Without
 *                 a reference (absolute mode) x_i = d_i, rounded the same way for a 16-bit slot.  NaN and inf in g
 *                 propagate; -0 + +0 is +0.  (slot, ref) pairs are the (in, out) pairs below.
 *              Encode (fa_mx8_encode, pure host arithmetic, the owner's side).  Per block, over its (at most 32)
 *              fp32 deltas:
 *              1. If any is NaN or +-inf: E = 255, every q = 0.
 *              2. m = max |delta|.  If m is 0: E = 0, every q = 0.
 *              3. Otherwise m = f 2^k with f in [0.5, 1) (frexp); t = k - 7 if f <= 127/128, else k - 6: the
 *                 smallest t with m 2^-t <= 127.  E = min(max(t + 133, 0), 254) and t = E - 133.
 *                 q_i = clamp(rint(delta_i 2^-t), -127, 127), computed in fp64 where the scaling is exact, ties to
 *                 even.  The encoder never emits -128.
 *              4. Error: for a block without E = 255, |delta_i - d_i| <= max(m / 127, 2^-134): the minimal t makes
 *                 the step below 2 m / 127, and saturation at E = 254 costs less than m / 128.
 *              5. Rounding to nearest is the library's encoder.  An owner may round stochastically: any (q, e) is
 *                 valid input to the decoder.
 *              Added without a new FA_ABI_VERSION: fa_mx8_expand_device with n == 0 touches no device and answers
 *              FA_OK -- that is how a caller probes for it.
 *   MX8 replies (fa_set_mx8_reply, fa_finalize_mx8, fa_copy_mx8, fa_mx8_encode_device): the other direction.  The new
 *              model goes back to the owners as an MX8 update against the model they were last sent, encoded on
 *              the GPU; the format and the decoder are those of MX8 receipts.  The reply is lossy, so the library
 *              continues from what the owners then hold, not from its own aggregate.
 *              Part state: `sent`, the model the owners last received -- per GPU the elements of its range, in the
 *              part's out dtype -- and whether it exists.
 *              Per reducing call of a part with the stage on:
 *              1. y is the part's output exactly as the call would leave it without the stage: after the noise
 *                 stage and the server optimizer, rounded to the out dtype.
 *              2. Bootstrap.  If `sent` does not exist: the output stays y, sent := y, the round has no codes.
 *              3. Otherwise, per element, delta_i = fl32(widen(y_i) - widen(sent_i)), one IEEE subtract, no
 *                 contraction.  The deltas are encoded by encode rules 1-3 of MX8 receipts, unchanged, into q and
 *                 e; the block of an element is its bucket index >> 5, whatever the shard.  The GPU's bytes are
 *                 those fa_mx8_encode gives for these deltas.  (The kernel takes E from the bit pattern of the
 *                 block's maximum: its exponent field, one more if the mantissa is above 0x7E0000, 0 up to the
 *                 subnormal 0x7F0000, held at 254 -- the same number as rule 3's frexp.)
 *              4. g'_i is decode rule 3 of (q, e) against sent, into the out dtype: fl32(widen(sent_i) +
 *                 fl32((float)q_i * s)), rounded once more for a 16-bit out dtype.  A block with E = 255 becomes
 *                 NaN throughout, as the decoder says, and stays NaN until fa_mx8_set_reference is called or the
 *                 stage is switched off and on (which drops `sent`: the next round is a bootstrap).  The round
 *                 reports its count of E = 255 blocks (fa_mx8_reply_stats).
 *              5. The part's device output becomes g', and sent := g'.  Everything that reads the part's output
 *                 after the call sees g': fa_copy_output, fa_finalize*, fa_output_crc32, fa_bucket_output, the
 *                 clip stage's reference update (clip rule 6) and the reference of MX8 receipts.  The server
 *                 optimizer's master and moments and the noise counter are not touched: the master keeps the
 *                 exact model, and the next round's delta, taken from the master's output against g', carries
 *                 this round's quantisation error into the next reply.
 *              6. Layout independence.  q, e and g' are the same bytes for any GPU count and any range
 *                 boundaries.  A block that lies in the ranges of several GPUs gets the byte maximum of their
 *                 partial scales -- exact, because E is non-decreasing in the block maximum and 255 dominates --
 *                 and the codes of its elements are taken under that scale (fa_mx8_encode_device's scales-only
 *                 and scales-given modes around the maximum).  A context never has such a block: its range shards
 *                 and pieces are cut at multiples of 64 elements, so no round has that extra wait, and the stage
 *                 refuses a range that starts inside a block (FA_ERR_STATE).
 *              Added without a new FA_ABI_VERSION: fa_mx8_encode_device with n == 0 touches no device and answers
 *              FA_OK -- that is how a caller probes for it.
 *   FA_F16     IEEE binary16 bits.  The fp32 result is rounded once to
 *              binary16, round-to-nearest-even: values that round beyond 65504
 *              become +-inf, results below 2^-14 become fp16 subnormals (never
 *              flushed), a NaN result is some quiet NaN (the payload is not
 *              specified).
 *   Dtype pairs (in -> out): f32 -> f32, f32 -> bf16, bf16 -> f32, bf16 -> bf16,
 *              f16 -> f16, f16 -> f32, f32 -> f16.  bf16 <-> f16 is refused with
 *              FA_ERR_ARG (fa_bucket_define, fa_reduce_device).
 *   FA_F16 was added without a new FA_ABI_VERSION (a new enum value is additive):
 *              a library without it answers FA_ERR_ARG ("bad dtype") to dtype 2,
 *              e.g. from fa_fill_uniform(NULL, 0, FA_F16, ...), which touches no
 *              device -- that is how a caller probes for fp16.
 */
#ifndef FEDAVG_FA_H_
#define FEDAVG_FA_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FA_ABI_VERSION 7

typedef struct fa_ctx fa_ctx; /* opaque: device slots, streams, pinned staging */

typedef enum { FA_F32 = 0, FA_BF16 = 1, FA_F16 = 2 /* IEEE binary16 */ } fa_dtype;
typedef enum { FA_FEDAVG = 0, FA_LITERAL = 1, FA_TRIMMED = 2 /* trimmed mean / median */ } fa_mode;
/* fa_set_trim / fa_trimmed_device: the largest valid trim, (D-1)/2 -- the coordinate-wise median. */
#define FA_TRIM_MEDIAN (-1)
/* Most clients of an FA_TRIMMED bucket (more: FA_ERR_ARG; a sort has no multi-pass form). */
#define FA_TRIMMED_MAX_CLIENTS 128
/* Most clients of a part with the Krum stage, and of fa_pairdist_device (more: FA_ERR_ARG). */
#define FA_KRUM_MAX_CLIENTS 128
/* Most clients of a part with the geomed stage, and of fa_geomed_pass_device; most Weiszfeld passes per round. */
#define FA_GEOMED_MAX_CLIENTS 128
#define FA_GEOMED_MAX_ITERS 64

typedef enum {
    FA_OK = 0,
    FA_ERR_ARG = -1,     /* bad argument (null pointer, size, dtype, slot) */
    FA_ERR_HIP = -2,     /* a HIP runtime call failed */
    FA_ERR_NOMEM = -3,   /* device or pinned allocation failed */
    FA_ERR_STATE = -4,   /* call out of order (e.g. finalize before any submit) */
    FA_ERR_NODEV = -5,   /* no usable gfx950 device */
    FA_ERR_ALIGN = -6,   /* pointer not 4-byte (f32) / 2-byte (bf16, f16) aligned */
    FA_ERR_NCCL = -7     /* an RCCL call failed (FA_SHARD_CLIENT_RS) */
} fa_status;

/* fa_create flags */
/* n_gpus > 1: GPU g owns elements [g*n/G, (g+1)*n/G) of every client bucket; bit-exact, no collective. */
#define FA_SHARD_RANGE 0x1
/* Client-sharded: GPU g holds whole buckets of clients [c_g, c_{g+1}) (contiguous, balanced), reduces them
 * into an fp32 partial, and an RCCL reduce-scatter over xGMI (one communicator per GPU, ncclCommInitAll in
 * this process) sums the partials piece by piece, overlapped with the reduction of the next piece
 * (fa_tuning.rs_chunks pieces; GPU g ends with block g of every piece, fa_rs_segments).  The summation
 * order changes: within 1e-6 of sum_k |w_k x_k| (bit-exact at n_gpus = 1).  A bf16 or fp16 output is the fp32
 * result rounded once to that type on each GPU after the exchange (so within one such rounding of that). */
#define FA_SHARD_CLIENT_RS 0x2
/* Accumulate on arrival (range layout, FedAvg): as soon as receipts 0..k-1 of a round are all in, their
 * ordered chain is enqueued (continued in an fp32 accumulator), so the phase end only reduces the
 * clients that came late or out of order.  Same bits as one chain. */
#define FA_ACCUMULATE_ON_ARRIVAL 0x4
/* Test only: accept a device id more than once (several shards of one context on one GPU), so the
 * multi-GPU host logic runs on a one-GPU box.  RCCL refuses two ranks on one device, so with
 * FA_SHARD_CLIENT_RS the reduce-scatter is replaced by its definition (shard g's block := the sum of the
 * GPUs' partials in ring order, starting at rank g + 1 and ending at rank g as a ring reduce-scatter
 * accumulates it; one device launch); everything else of the layout is unchanged. */
#define FA_TEST_SHARED_DEVICE 0x100

int fa_version(void);
const char* fa_last_error(void); /* thread-local; "" when the last call succeeded */
int fa_device_count(int* out);   /* visible HIP devices */

/* Replaces the aggregator's state construction: systemAPI sys_(true, -1, ...)
 * + refactor() -> init_model_sate (aggregator.cpp:47,53; systemAPI.cpp:17-38).
 * Uses devices 0..n_gpus-1. */
int fa_create(fa_ctx** out, int n_gpus, int flags);
/* Same on an explicit device list (e.g. {LOCAL_RANK} for one process per GPU).  Every id once
 * (FA_SHARD_CLIENT_RS needs distinct devices for its RCCL communicators). */
int fa_create_ex(fa_ctx** out, const int* device_ids, int n_gpus, int flags);
void fa_destroy(fa_ctx* ctx);

/* One reduced bucket = the flattened named_parameters() of one model part
 * (model_part 1 -> parts[0].layers[0], aggregator.cpp:64; model_part m >= 2 ->
 * parts[1].layers[m-2], :118).  Allocates n_clients device slots per GPU. */
/* in / out: one of the dtype pairs above (bf16 <-> f16: FA_ERR_ARG, naming both). */
int fa_bucket_define(fa_ctx* ctx, int part_id, size_t n_elems, fa_dtype in, fa_dtype out, int n_clients,
                     fa_mode mode);
/* kTrainSize_10 of aggregator.cpp:48 for FA_LITERAL buckets (default 1000). */
int fa_set_literal_divisor(fa_ctx* ctx, int part_id, float divisor);
/* Trim t of FA_TRIMMED buckets: FA_TRIM_MEDIAN (the default) or 0 <= t with 2t < D.  part_id as for
 * fa_set_literal_divisor: < 0 sets the context-wide default of parts defined later (checked against D
 * when a part is defined), else the part's own trim from its next reduction on.  FA_ERR_ARG (naming D and
 * trim) when trim < -1 or 2 trim >= D.
 * An FA_TRIMMED bucket: at most FA_TRIMMED_MAX_CLIENTS clients; not on an FA_SHARD_CLIENT_RS context (the
 * rule needs every client's value of an element on one GPU); FA_ACCUMULATE_ON_ARRIVAL leaves it non-eager
 * (nothing is reduced before the phase end, as for FA_LITERAL); its receipts are never kept host-side
 * (fa_submit_pinned copies them in, fa_bucket_host_read says 0); every client must have submitted before
 * fa_finalize*.  fa_reduce_part(s) (h_weights ignored; its own launch, never in the segment table),
 * fa_finalize*, fa_copy_output, fa_output_crc32, range shards and range pieces work as for FA_FEDAVG.
 * fa_sync_part and fa_sync_device keep their FedAvg meaning: fa_sync_part refuses a trimmed part. */
int fa_set_trim(fa_ctx* ctx, int part_id, int trim);

/* Replaces one receipt: torch::load into the global module + the per-parameter
 * update (aggregator.cpp:63-88 / :117-142).  Copies host_src (n_elems of the
 * bucket dtype, caller-owned, reusable on return) through ctx pinned staging
 * to the device slot asynchronously.  weight = w_k for FA_FEDAVG (ignored for
 * FA_LITERAL).  Submitting a slot twice in one round overwrites it. */
int fa_submit(fa_ctx* ctx, int part_id, int client_slot, const void* host_src, float weight);
/* Same, but host_src is pinned (hipHostMalloc'd / registered) memory that the
 * caller keeps unchanged until fa_finalize returns: no staging copy.
 * Small receipts are read where they are: on a one-GPU range context without
 * FA_ACCUMULATE_ON_ARRIVAL, a part whose D receipts total at most
 * FA_HOST_READ_MAX_BYTES keeps element-aligned pinned receipts in place, and the
 * fa_finalize* that ends the round has its kernels read them over PCIe -- with
 * FA_HOST_PINNED straight into the pinned destination: one stream round trip for
 * the phase (a small model's round is bound by round trips, not bytes).  Same
 * bits.  Calls before it that need the device slots (fa_reduce_part(s),
 * fa_sync_part, fa_bucket_slot/_piece, a pageable submit to the part) copy the
 * kept receipts in first.  A finalize that wrote a pinned destination this way
 * leaves the part's device output (fa_bucket_output) as it was, and
 * fa_copy_output of the part then fails with FA_ERR_STATE until its next
 * reduction.  fa_bucket_host_read tells whether a part's round is being kept
 * this way.  FA_HOST_READ=0 in the environment turns this off. */
#define FA_HOST_READ_MAX_BYTES (1u << 20)
int fa_submit_pinned(fa_ctx* ctx, int part_id, int client_slot, const void* host_src, float weight);

/* Same as fa_submit for a receipt scattered over n_segments host pieces whose
 * concatenation is the bucket (e.g. the parameter records of a torch::save
 * archive mapped in place, in named_parameters() order): gathered straight into
 * the pinned staging chunks, no intermediate flat copy. */
int fa_submit_gather(fa_ctx* ctx, int part_id, int client_slot, int n_segments, const void* const* srcs,
                     const size_t* bytes, float weight);
/* Zero-copy ingest: the segments lie in pinned memory (fa_host_alloc), e.g. the
 * parameter records of an archive inside a frame the network layer received
 * into a pinned buffer, and stay unchanged until fa_finalize* returns.  The
 * H2D DMA runs from them directly, no staging copy. */
int fa_submit_gather_pinned(fa_ctx* ctx, int part_id, int client_slot, int n_segments, const void* const* srcs,
                            const size_t* bytes, float weight);

/* Streaming ingest: a receipt handed over while its frame is still arriving (network_layer.cpp:48-65 reads
 * the whole frame first; aggregator.cpp:63-64 then decodes it).  fa_submit_piece_pinned enqueues the H2D
 * DMA of bytes [byte_offset, byte_offset + bytes) of the bucket (e.g. one parameter record, as soon as its
 * bytes are in) from pinned memory the caller keeps unchanged until fa_finalize* returns.  The slot counts
 * as the client's receipt only after fa_submit_commit (weight as for fa_submit); pieces never committed are
 * overwritten by the slot's next submit.  A piece overlapping one already sent replaces those bytes. */
int fa_submit_piece_pinned(fa_ctx* ctx, int part_id, int client_slot, size_t byte_offset, const void* host_src,
                           size_t bytes);
int fa_submit_commit(fa_ctx* ctx, int part_id, int client_slot, float weight);

/* Replaces the end of a phase: the reduced module handed to new_message()
 * (aggregator.cpp:96-106 / :153-166).  Waits for the submits, reduces on every
 * GPU, copies the result (out dtype) to host_dst and resets the round. */
int fa_finalize(fa_ctx* ctx, int part_id, void* host_dst);
/* Same, scattering the result over n_segments host pieces (e.g. the parameter
 * records of the reply archive inside the outgoing frame, aggregator.cpp:96-101
 * + network_layer.cpp:305-313).  flags: FA_HOST_PINNED = every segment is pinned
 * memory, DMA'd into directly; 0 = pageable, copied through the pinned chunks. */
#define FA_HOST_PINNED 0x1
int fa_finalize_gather(fa_ctx* ctx, int part_id, int n_segments, void* const* dsts, const size_t* bytes,
                       int flags);

/* Pinned (page-locked, every device can DMA it) host memory, for frame buffers
 * that feed fa_submit_gather_pinned / fa_finalize_gather(FA_HOST_PINNED). */
int fa_host_alloc(size_t bytes, void** out);
int fa_host_free(void* p);

/* Device-resident round (the data path with buckets already in HBM, e.g. a
 * zero-copy ingest that lands receipts straight in the slots): reduce the
 * part's slots into its device output on every GPU, no host copies.
 * h_weights: D floats, NULL = the weights given to fa_submit.  hip_stream:
 * NULL = ctx compute streams; non-NULL only for a single-GPU ctx.  Async. */
int fa_reduce_part(fa_ctx* ctx, int part_id, const float* h_weights, void* hip_stream);
/* Device pointer of client slot `client_slot` on GPU `gpu` (n_elems elements of
 * the input dtype, covering bucket elements [elem_offset, elem_offset+n_elems);
 * FA_SHARD_CLIENT_RS: only the GPU holding the client, whole bucket).  Slots of one bucket share one allocation
 * with a small per-slot byte skew (fa_tuning.slot_skew) so that the wave's
 * simultaneous loads spread over HBM channels. */
int fa_bucket_slot(fa_ctx* ctx, int part_id, int gpu, int client_slot, void** d_ptr, size_t* n_elems,
                   size_t* elem_offset);
/* Range layout: a GPU whose client slots would span more than 48 GiB holds them as pieces of <= 16 GiB of
 * slots each (fa_tuning.piece_span_kib / piece_split_kib, taken at fa_bucket_define), reduced
 * one launch per piece.  fa_bucket_slot then fails (FA_ERR_STATE); a slot is written piece by piece instead.
 * n_pieces: 1 for every other part. */
int fa_bucket_pieces(fa_ctx* ctx, int part_id, int gpu, int* n_pieces);
/* Piece `piece` of client slot `client_slot` on GPU `gpu`: n_elems elements of the input dtype covering
 * bucket elements [elem_offset, elem_offset+n_elems). */
int fa_bucket_piece(fa_ctx* ctx, int part_id, int gpu, int piece, int client_slot, void** d_ptr, size_t* n_elems,
                    size_t* elem_offset);
/* The part's device output on GPU `gpu` (range: its shard, `out` dtype; rs: its fp32 shard, the blocks
 * fa_rs_segments lists, concatenated). */
int fa_bucket_output(fa_ctx* ctx, int part_id, int gpu, void** d_ptr);
/* This round's receipts so far and how many leading client slots are already reduced
 * (FA_ACCUMULATE_ON_ARRIVAL; n_reduced == D once the round's result is ready). */
int fa_bucket_progress(fa_ctx* ctx, int part_id, int* n_submitted, int* n_reduced);
/* Whether the part's round so far is kept host-side to be read in place (fa_submit_pinned, small receipts):
 * *kept = 1 when every receipt its reduction reads is held that way, so the fa_finalize* ending the round
 * reduces them itself (a caller then skips fa_reduce_parts for it, which would copy them in first); else 0. */
int fa_bucket_host_read(fa_ctx* ctx, int part_id, int* kept);
/* Batched device-resident reduction of several parts (e.g. all last-part layers of a phase,
 * aggregator.cpp:108-150): one launch per GPU covers every part that is FedAvg, range-laid-out, has at
 * most 128 clients and is below the phased kernel's size (a segment table: one bucket per segment,
 * the same ordered chain, the same bits); larger parts get their own launch.  h_weights: NULL or one
 * entry per part (NULL entry = the weights given to fa_submit).  A following fa_finalize* of these
 * parts only copies the result out.  Async on hip_stream (NULL = ctx compute streams). */
int fa_reduce_parts(fa_ctx* ctx, int n_parts, const int* part_ids, const float* const* h_weights, void* hip_stream);
/* D2H of the part's current device output (after fa_reduce_part), waiting for it.  FA_ERR_STATE when the
 * part has no device output: never reduced, or its last round was read in place straight into a pinned
 * reply (fa_submit_pinned). */
int fa_copy_output(fa_ctx* ctx, int part_id, void* host_dst);
/* CRC-32 (zlib's: IEEE 802.3, reflected, initial and final inversion) of consecutive byte segments of the
 * part's current device output: segment k = bytes [sum_{j<k} bytes[j], + bytes[k]) of the reduced bucket in
 * its out dtype; the segments cover it exactly.  Computed on the GPU(s) holding the output, from HBM: for the
 * zip records of a reply built around the reduced parameters (aggregator.cpp:96-101 hands the module to
 * torch::save, which writes a CRC-32 per record), so the host need not read the reply back.  Waits for the
 * reduction and returns with the CRCs.  FA_ERR_STATE when the part has no device output (never reduced, or
 * its last round was read in place straight into a pinned reply). */
int fa_output_crc32(fa_ctx* ctx, int part_id, int n_segments, const size_t* bytes, uint32_t* crcs);
/* Wait for all copy and compute work of the ctx. */
int fa_sync(fa_ctx* ctx);

/* Raw device entry for benches and device-resident callers: reduce D client
 * buckets already resident on device `gpu` into d_out.  d_clients[k] are device
 * pointers, h_weights a host array of D floats (copied into kernel arguments,
 * any D >= 1).  d_init (nullable, fp32, n) continues an earlier chain: acc
 * starts at d_init[i] instead of +0 (used to split clients across launches or
 * GPUs bit-exactly).  Enqueued on hip_stream (a hipStream_t; NULL = the
 * ctx's compute stream of `gpu`); returns without synchronizing.  ctx may be
 * NULL except for a bf16 or fp16 output with D > 128 (needs ctx scratch:
 * FA_ERR_ARG without one).  A bf16 <-> f16 pair: FA_ERR_ARG.  mode FA_TRIMMED: FA_ERR_ARG (the
 * signature has no room for a trim and d_init no meaning there; use fa_trimmed_device). */
int fa_reduce_device(fa_ctx* ctx, int gpu, const void* const* d_clients, const float* h_weights, int D, size_t n,
                     fa_dtype in, void* d_out, fa_dtype out, fa_mode mode, const float* d_init, void* hip_stream);

/* The same for FA_TRIMMED: the trimmed mean (trim: FA_TRIM_MEDIAN or 0 <= 2 trim < D) of D client buckets
 * resident on device `gpu` into d_out.  ctx may be NULL (then `gpu` is the HIP device).  Every argument is
 * checked before any device call: D in 1..FA_TRIMMED_MAX_CLIENTS, trim, the dtype pair, and for n > 0 null
 * pointers and element alignment; with n == 0 and valid arguments it returns FA_OK without touching a
 * device.  Async on hip_stream (NULL = the ctx's compute stream of `gpu`, or the null stream). */
int fa_trimmed_device(fa_ctx* ctx, int gpu, const void* const* d_clients, int D, size_t n, fa_dtype in, void* d_out,
                      fa_dtype out, int trim, void* hip_stream);

/* Server optimizer: what is done with the round's aggregate (the header comment, "Server optimizer"). */
typedef enum { FA_OPT_NONE = 0, FA_OPT_MOMENTUM = 1, FA_OPT_ADAGRAD = 2, FA_OPT_ADAM = 3, FA_OPT_YOGI = 4 } fa_opt_rule;
typedef struct {
    int rule;                    /* an fa_opt_rule */
    float lr, beta1, beta2, tau; /* beta2: FA_OPT_ADAM / FA_OPT_YOGI; tau: the adaptive rules */
} fa_server_opt;
/* Gives a part a server-optimizer stage (part_id >= 0), or sets the context default that FA_FEDAVG and
 * FA_TRIMMED parts defined later take (part_id < 0; FA_LITERAL parts ignore it).  Calling again with the same
 * rule keeps the state and changes the hyperparameters (a decaying server learning rate); a different rule
 * keeps x and zeroes m and v (a round already reduced stays reduced: one step per round); NULL or
 * FA_OPT_NONE removes the stage and frees its state (a part that took the context default on an
 * FA_ACCUMULATE_ON_ARRIVAL context was defined non-eager and stays so).  The state is per
 * GPU and covers the elements that GPU's output covers (a range shard: [off, off + cnt)): 2 or 3 fp32 arrays
 * (plus an fp32 aggregate buffer for a 16-bit output) that live until the part or the context goes;
 * FA_ERR_NOMEM when they cannot be allocated.  FA_ERR_ARG, naming the field: rule outside 0..4, lr not finite
 * or < 0, beta1 outside [0, 1), beta2 outside [0, 1) (Adam, Yogi), tau not finite or <= 0 (the adaptive
 * rules), an FA_LITERAL part, an FA_SHARD_CLIENT_RS context (its aggregate is not bit-specified).
 * The step happens once per reducing call: fa_reduce_part, fa_reduce_parts (its own launch, never in the
 * segment table) or the fa_finalize* that reduces the round; each reduces in fp32 (an f32 part into its
 * output, a 16-bit part into an fp32 buffer of its own) and runs the stage on the same stream into the part's
 * output.  On such a part fa_reduce_part needs every client submitted and marks the round reduced, so a
 * following fa_finalize* only copies out; calling it twice takes two steps.  The part is never kept host-side
 * (fa_bucket_host_read says 0) and FA_ACCUMULATE_ON_ARRIVAL leaves it non-eager.  fa_sync_part keeps its
 * meaning and takes no step; fa_copy_output, fa_output_crc32, range shards and range pieces read the part's
 * output and work unchanged. */
int fa_set_server_opt(fa_ctx* ctx, int part_id, const fa_server_opt* opt);
/* The stage's state as whole-bucket host arrays of n fp32, scattered to / gathered from the GPUs' shards; any
 * pointer may be NULL to skip that array, v is ignored for FA_OPT_MOMENTUM.  set with an x gives the part a
 * master (no bootstrap); get waits for the part's pending work (not when only steps is asked for).  FA_ERR_STATE on a part without a stage. */
/* The stage a part has (rule FA_OPT_NONE: none), or with part_id < 0 the context default. */
int fa_get_server_opt(fa_ctx* ctx, int part_id, fa_server_opt* opt);
int fa_server_opt_set_state(fa_ctx* ctx, int part_id, const float* x, const float* m, const float* v, uint64_t steps);
int fa_server_opt_get_state(fa_ctx* ctx, int part_id, float* x, float* m, float* v, uint64_t* steps);
/* One step on raw device pointers (no bootstrap): d_avg, d_x, d_m, d_v of n fp32 on device `gpu`; d_v may be
 * NULL for FA_OPT_MOMENTUM; d_out (n of `out`) may be NULL (states only) or d_avg itself for FA_F32.  ctx may
 * be NULL (then `gpu` is the HIP device).  Every argument is checked before any device call: the rule (not
 * FA_OPT_NONE) and hyperparameters as above, the out dtype, and for n > 0 null pointers and element alignment
 * (FA_ERR_ALIGN); with n == 0 and valid arguments it returns FA_OK without touching a device.  Async on
 * hip_stream (NULL = the ctx's compute stream of `gpu`, or the null stream). */
int fa_server_opt_device(fa_ctx* ctx, int gpu, const fa_server_opt* opt, const float* d_avg, float* d_x, float* d_m,
                         float* d_v, size_t n, void* d_out, fa_dtype out, void* hip_stream);

/* Clip stage: per-client L2 norm clipping of an FA_FEDAVG part's updates (the header comment, "Clip stage").
 * Gives a part the stage with bound max_norm > 0 (part_id >= 0; calling again changes the bound and keeps the
 * reference), or sets the context default that FA_FEDAVG parts defined later take (part_id < 0).  max_norm == 0
 * removes the stage and frees its arrays (per GPU: the fp32 reference over the elements that GPU's output
 * covers, plus an fp32 buffer of that size for a 16-bit input).  FA_ERR_ARG, naming the cause: max_norm not
 * finite or < 0, an FA_LITERAL or FA_TRIMMED part, an FA_SHARD_CLIENT_RS context.  FA_ERR_NOMEM when the arrays
 * cannot be allocated.  Like a part with a server optimizer (the two compose, in either call order), a clipped
 * part is never kept host-side (fa_bucket_host_read says 0), FA_ACCUMULATE_ON_ARRIVAL leaves it non-eager, it
 * gets its own launches in fa_reduce_parts (never the segment table), and a reducing call (fa_reduce_part,
 * fa_reduce_parts, the fa_finalize* that reduces the round) needs every client submitted; fa_reduce_part marks
 * the round reduced, so a following fa_finalize* only copies out.  Such a call waits on the host for the norm
 * pass before it enqueues the chain: one stream round trip.  Range shards and range pieces work. */
int fa_set_clip(fa_ctx* ctx, int part_id, float max_norm);
/* The reference as a whole-bucket host array of n fp32, scattered to / gathered from the GPUs' shards.  set with
 * g == NULL drops the reference: the next round bootstraps.  FA_ERR_STATE on a part without the stage, and from
 * get on a part without a reference.  Both wait for the part's pending work. */
int fa_clip_set_reference(fa_ctx* ctx, int part_id, const float* g);
int fa_clip_get_reference(fa_ctx* ctx, int part_id, float* g);
/* What the part's last reducing call did: sumsq[k] = Q_k, scales[k] = s_k (0 for an excluded client),
 * included[k] = 0 / 1, *n_clipped = the included clients with s_k < 1.  Each array holds D entries; any pointer
 * may be NULL.  After a bootstrap round: Q_k = 0, s_k = 1, all included.  FA_ERR_STATE on a part without the
 * stage or never reduced with it. */
int fa_clip_get_round(fa_ctx* ctx, int part_id, double* sumsq, float* scales, int* included, int* n_clipped);
/* Rule 2 of the stage, pure host arithmetic: the scale of a client whose squared distance is sumsq under the
 * bound max_norm; *excluded (nullable) = 1 and the result 0 when sqrt(sumsq) is NaN or +inf. */
float fa_clip_scale(double sumsq, float max_norm, int* excluded);
/* Rule 1 on raw device pointers: h_sumsq[k] = Q_k of the D client buckets (n elements of `in`) against d_ref (n
 * fp32) on device `gpu`, any D >= 1.  ctx may be NULL (then `gpu` is the HIP device).  Every argument is checked
 * before any device call: D, the dtype, h_sumsq, and for n > 0 null pointers and element alignment
 * (FA_ERR_ALIGN); with n == 0 and valid arguments it touches no device, writes D zeros and answers FA_OK.
 * Otherwise it enqueues on hip_stream (NULL = the ctx's compute stream of `gpu`, or the null stream), waits for
 * it and returns the D sums. */
int fa_clip_sumsq_device(fa_ctx* ctx, int gpu, const void* const* d_clients, int D, size_t n, fa_dtype in,
                         const float* d_ref, double* h_sumsq, void* hip_stream);

/* Krum stage: distance-based selection of an FA_FEDAVG part's owners (the header comment, "Krum stage").  Gives a
 * part the stage with parameters f and m (part_id >= 0; calling again changes them), or sets the context default
 * that FA_FEDAVG parts defined later take (part_id < 0; checked against D when such a part is defined, where a
 * misfit makes fa_bucket_define fail).  m == -1 means D - f; m == 0 removes the stage.  FA_ERR_ARG, naming the
 * cause: f < 0 or m < -1, f or m that do not fit the part's D (0 <= f, 2 f + 2 < D, 1 <= m <= D - f), D >
 * FA_KRUM_MAX_CLIENTS, an FA_LITERAL or FA_TRIMMED part, an FA_SHARD_CLIENT_RS context, a part (or context
 * default) that has the clip stage -- and fa_set_clip on a Krum part: the two do not compose.  A server optimizer
 * composes, in either call order.  Like the other stage parts a Krum part is never kept host-side
 * (fa_bucket_host_read says 0), FA_ACCUMULATE_ON_ARRIVAL leaves it non-eager, it gets its own launches in
 * fa_reduce_parts, and a reducing call needs every client submitted (FA_ERR_STATE otherwise); fa_reduce_part marks
 * the round reduced.  Such a call waits on the host for the distance pass before it enqueues the chain: one stream
 * round trip.  Range shards and range pieces work.  The stage keeps no state across rounds. */
int fa_set_krum(fa_ctx* ctx, int part_id, int f, int m);
/* What the part's last reducing call did: dist = the D x D matrix Q (row-major), scores[k] = S_k, selected[k] =
 * 0 / 1, *n_selected = how many are selected.  Any pointer may be NULL.  FA_ERR_STATE on a part without the stage
 * or never reduced with it. */
int fa_krum_get_round(fa_ctx* ctx, int part_id, double* dist, double* scores, int* selected, int* n_selected);
/* Rules 2-3 of the stage, pure host arithmetic, usable without a device: the scores and the selection flags (D
 * entries each, either may be NULL) of the D x D row-major matrix dist under f and m (-1: D - f).  FA_ERR_ARG for
 * a null dist and for D, f, m as in fa_set_krum.  A caller that wants Krum over a whole model sums the matrices of
 * its parts, selects once and runs fa_reduce_device with the weights of fa_krum_weights. */
int fa_krum_select(const double* dist, int D, int f, int m, double* scores, int* selected, int* n_selected);
/* Rule 4, pure host arithmetic: w_out[k] = w'_k for every k (the deselected ones included: they do not enter the
 * chain). */
int fa_krum_weights(const float* w, const int* selected, int D, float* w_out);
/* Rule 1 on raw device pointers: h_dist (D * D doubles, row-major) = the matrix Q of the D client buckets (n
 * elements of `in`) on device `gpu`, 1 <= D <= FA_KRUM_MAX_CLIENTS.  ctx may be NULL (then `gpu` is the HIP
 * device).  Every argument is checked before any device call: D, the dtype, h_dist, and for n > 0 null pointers
 * and element alignment (FA_ERR_ALIGN); with n == 0 and valid arguments it touches no device, writes D * D zeros
 * and answers FA_OK.  Otherwise it enqueues on hip_stream (NULL = the ctx's compute stream of `gpu`, or the null
 * stream), waits for it and returns the matrix. */
int fa_pairdist_device(fa_ctx* ctx, int gpu, const void* const* d_clients, int D, size_t n, fa_dtype in, double* h_dist,
                       void* hip_stream);

/* Bulyan stage: iterated Krum, then a median-centred mean, on an FA_TRIMMED part (the header comment, "Bulyan
 * stage").  Gives a part the stage with f owners assumed Byzantine (part_id >= 0; calling again changes f), or sets
 * the context default that FA_TRIMMED parts defined later take (part_id < 0; checked against D when such a part is
 * defined, where a misfit makes fa_bucket_define fail).  f == -1 removes the stage: the part is a plain FA_TRIMMED
 * part with its trim again.  FA_ERR_ARG, naming the cause: f < -1, an f that does not fit the part's D (4 f + 3 <=
 * D), a part that is not FA_TRIMMED, an FA_SHARD_CLIENT_RS context.  The server optimizers and the noise stage
 * compose, in either call order; the clip and Krum stages are FA_FEDAVG stages and never meet it.  Like the other
 * stage parts a Bulyan part gets its own launches in fa_reduce_parts and fa_reduce_part marks the round reduced; like
 * every FA_TRIMMED part it is never eager or kept host-side and needs every client submitted.  A reducing call waits
 * on the host for the distance pass before it enqueues the centred mean: one stream round trip.  Range shards and
 * range pieces work. */
int fa_set_bulyan(fa_ctx* ctx, int part_id, int f);
/* What the part's last reducing call did: dist = the D x D matrix Q (row-major); order[i] and pick_scores[i], i <
 * *n_selected, = the i-th pick and the score S it was picked with (D entries each; the unused ones hold -1 and
 * +inf); selected[k] = 0 / 1 (D entries).  Any pointer may be NULL.  FA_ERR_STATE on a part without the stage or
 * never reduced with it. */
int fa_bulyan_get_round(fa_ctx* ctx, int part_id, double* dist, int* order, double* pick_scores, int* selected,
                        int* n_selected);
/* Rule 2 of the stage, pure host arithmetic, usable without a device: the picks of the D x D row-major matrix dist
 * under f, arrays as in fa_bulyan_get_round (any but dist may be NULL).  FA_ERR_ARG for a null dist and for D and f
 * as in fa_set_bulyan.  A caller that wants Bulyan over a whole model sums the matrices of its parts, selects once and
 * runs fa_centered_device over the picked owners' buckets with keep = max(1, *n_selected - 2 f). */
int fa_bulyan_select(const double* dist, int D, int f, int* order, double* pick_scores, int* selected, int* n_selected);
/* Rule 4 on raw device pointers: per element the mean of the `keep` values closest to the median of D client
 * buckets resident on device `gpu`, into d_out; D in 1..FA_TRIMMED_MAX_CLIENTS, keep in 1..D.  ctx may be NULL (then
 * `gpu` is the HIP device).  Every argument is checked before any device call: D, keep, the dtype pair, and for n >
 * 0 null pointers and element alignment; with n == 0 and valid arguments it returns FA_OK without touching a device.
 * Async on hip_stream (NULL = the ctx's compute stream of `gpu`, or the null stream). */
int fa_centered_device(fa_ctx* ctx, int gpu, const void* const* d_clients, int D, size_t n, fa_dtype in, void* d_out,
                       fa_dtype out, int keep, void* hip_stream);

/* Geomed stage: the geometric median of an FA_FEDAVG part's owners by smoothed Weiszfeld iterations (the header
 * comment, "Geomed stage").  Gives a part the stage with T = iters passes and the smoothing floor nu (part_id >= 0;
 * calling again changes them), or sets the context default that FA_FEDAVG parts defined later take (part_id < 0;
 * checked against D when such a part is defined, where a misfit makes fa_bucket_define fail).  iters == 0 removes the
 * stage (nu is then ignored).  FA_ERR_ARG, naming the cause: iters outside 0..FA_GEOMED_MAX_ITERS, nu not finite or
 * <= 0, D > FA_GEOMED_MAX_CLIENTS, an FA_LITERAL or FA_TRIMMED part, an FA_SHARD_CLIENT_RS context, a part (or context
 * default) that has the clip or the Krum stage -- and fa_set_clip or fa_set_krum on a geomed part: they do not compose.
 * The server optimizers and the noise stage compose, in either call order.  Like the other stage parts a geomed part
 * is never kept host-side (fa_bucket_host_read says 0), FA_ACCUMULATE_ON_ARRIVAL leaves it non-eager, it gets its own
 * launches in fa_reduce_parts, and a reducing call needs every client submitted (FA_ERR_STATE otherwise);
 * fa_reduce_part marks the round reduced.  Such a call waits on the host after each of its T passes (T + 1 on a
 * round with a non-finite bucket) and then enqueues the chain.  Range shards and range pieces work.  The stage keeps
 * no state across rounds. */
int fa_set_geomed(fa_ctx* ctx, int part_id, int iters, float nu);
/* The stage a part has (*iters == 0: none), or with part_id < 0 the context default.  Either pointer may be NULL. */
int fa_get_geomed(fa_ctx* ctx, int part_id, int* iters, float* nu);
/* The whole trace of the part's last reducing call.  *n_passes = the valid passes P <= T (a voided pass is not
 * reported); sumsq[t * D + k] = Q^t_k for t < P (room for FA_GEOMED_MAX_ITERS * D; 0 for a client not in pass t);
 * weights[t * D + k] = alpha^t_k for t <= P, the last row the final chain's weights (room for
 * (FA_GEOMED_MAX_ITERS + 1) * D; 0 for a client excluded by then); included[k] = the final flags (D entries);
 * objective[t] = sum_k (double)w_k N^t_k over the clients included at pass t, in client order (room for
 * FA_GEOMED_MAX_ITERS).  Any pointer may be NULL.  FA_ERR_STATE on a part without the stage or never reduced with it. */
int fa_geomed_get_round(fa_ctx* ctx, int part_id, int* n_passes, double* sumsq, float* weights, int* included,
                        double* objective);
/* Rules 3-4 of the stage, pure host arithmetic, usable without a device: included (D flags, in and out) loses the
 * clients whose sqrt(sumsq[k]) is NaN or +inf; w_out[k] = alpha_k for the clients still included, 0 for the others.
 * w are the round's own weights: a client whose w_k is not > 0 loses its flag too, and W is the fp64 sum of every
 * w_k > 0 in client order whatever the flags say -- the mass of the owners that entered the round stays W when one
 * of them is excluded on the way.  Entries of sumsq of clients not included are not read.  The stage's
 * objective[t] is sum_k (double)w_k N_k over the clients still included after rule 3.  FA_ERR_ARG for a null
 * pointer, D < 1, nu not finite or <= 0. */
int fa_geomed_weights(const float* w, const double* sumsq, int* included, int D, float nu, float* w_out);
/* Rule 1 on raw device pointers: over the D client buckets (n elements of `in`) on device `gpu`, 1 <= D <=
 * FA_GEOMED_MAX_CLIENTS, with the weights h_weights (D floats, host): h_sumsq[k] = Q_k against the chain v of all D
 * clients, h_nonfinite[k] = B_k (D doubles each, host), and, if d_v is not NULL, d_v (n fp32, device) = v.  ctx may be
 * NULL (then `gpu` is the HIP device).  Every argument is checked before any device call: D, the dtype, h_weights,
 * h_sumsq, h_nonfinite, and for n > 0 null pointers and element alignment (FA_ERR_ALIGN); with n == 0 and valid
 * arguments it touches no device, writes 2 D zeros and answers FA_OK.  Otherwise it enqueues on hip_stream (NULL = the
 * ctx's compute stream of `gpu`, or the null stream), waits for it and returns the 2 D numbers. */
int fa_geomed_pass_device(fa_ctx* ctx, int gpu, const void* const* d_clients, const float* h_weights, int D, size_t n,
                          fa_dtype in, float* d_v, double* h_sumsq, double* h_nonfinite, void* hip_stream);

/* Noise stage: Gaussian noise on a part's fp32 aggregate (the header comment, "Noise stage").  Gives a part the
 * stage with standard deviation stddev > 0 and the seed (part_id >= 0; the part id is the stream; calling again
 * changes stddev and seed and keeps the round counter), or sets the context default that FA_FEDAVG and FA_TRIMMED
 * parts defined later take (part_id < 0; FA_LITERAL parts ignore it).  stddev == 0 removes the stage (and the fp32
 * aggregate buffer of a 16-bit part, unless a server optimizer needs it); a stage given anew starts at round 0.
 * FA_ERR_ARG, naming the cause: stddev not finite or < 0, an FA_LITERAL part, an FA_SHARD_CLIENT_RS context (its
 * aggregate is not bit-specified).  FA_ERR_NOMEM when the buffer cannot be allocated.  The stage composes with the
 * clip stage, the Krum stage, the server optimizers and FA_TRIMMED, in any call order, and with range shards and
 * range pieces.  Like the other stage parts a noise part is never kept host-side (fa_bucket_host_read says 0),
 * FA_ACCUMULATE_ON_ARRIVAL leaves it non-eager, it gets its own launches in fa_reduce_parts, and a reducing call
 * needs every client submitted (FA_ERR_STATE otherwise); fa_reduce_part marks the round reduced.  Each reducing
 * call uses the part's round counter and then adds 1 to it: calling fa_reduce_part twice draws two noises. */
int fa_set_noise(fa_ctx* ctx, int part_id, float stddev, uint64_t seed);
/* The stage a part has (*stddev == 0: none), or with part_id < 0 the context default.  Either pointer may be NULL. */
int fa_get_noise(fa_ctx* ctx, int part_id, float* stddev, uint64_t* seed);
/* The round counter the part's next reducing call uses, in 0 .. 2^32 (2^32: that call fails with FA_ERR_STATE).
 * set: round <= 2^32, to replay a round or to continue a sequence after a restart.  FA_ERR_STATE on a part without
 * the stage. */
int fa_noise_get_round(fa_ctx* ctx, int part_id, uint64_t* round);
int fa_noise_set_round(fa_ctx* ctx, int part_id, uint64_t round);
/* Rules 1-4 on raw device pointers: d_out[i] (n of `out`, one rounding) = fl(d_avg[i] + fl(stddev z_{idx0 + i})) over
 * the n fp32 of d_avg on device `gpu`; d_out may be d_avg itself for FA_F32.  ctx may be NULL (then `gpu` is the HIP
 * device).  Every argument is checked before any device call: stddev (finite, > 0), the out dtype, idx0 + n < 2^64,
 * and for n > 0 null pointers and element alignment (FA_ERR_ALIGN); with n == 0 and valid arguments it returns FA_OK
 * without touching a device.  Async on hip_stream (NULL = the ctx's compute stream of `gpu`, or the null stream). */
int fa_noise_device(fa_ctx* ctx, int gpu, const float* d_avg, size_t n, void* d_out, fa_dtype out, float stddev,
                    uint64_t seed, uint32_t stream, uint32_t round, uint64_t idx0, void* hip_stream);
/* Rules 1-4's normals, pure host arithmetic, usable without a device: z[0, n) = the unit normals of elements idx0 ..
 * idx0 + n - 1 under (seed, stream, round), the bits the kernel adds (built without contraction: also on a host
 * with FMA units).  To audit a round: out == fl(a + fl(stddev z)). */
int fa_noise_host(uint64_t seed, uint32_t stream, uint32_t round, uint64_t idx0, size_t n, float* z);

/* MX8 receipts (the header comment, "MX8 receipts"): block-scaled int8 updates, expanded on the GPU. */
#define FA_MX8_BLOCK 32
/* ceil(n / 32): the bytes of e for a bucket of n elements. */
size_t fa_mx8_scale_bytes(size_t n);
/* The library's encoder, pure host arithmetic, usable without a device: the n fp32 deltas into q (n bytes) and e
 * (fa_mx8_scale_bytes(n) bytes), block b = elements [32 b, 32 b + 32). */
int fa_mx8_encode(const float* delta, size_t n, int8_t* q, uint8_t* e);
/* The decoder, pure host arithmetic: d[i] = the delta of bucket element idx0 + i, q[i] its code and e[0] the scale of
 * block idx0 >> 5 (e holds the scales of blocks idx0 >> 5 .. (idx0 + n - 1) >> 5).  The kernel's own arithmetic. */
int fa_mx8_decode(const int8_t* q, const uint8_t* e, size_t n, uint64_t idx0, float* d);
/* Decode rule 3 on raw device pointers: d_dst[i] (n of dst_dtype) = fl(widen(d_ref[i]) + d_i), or d_i with d_ref NULL
 * (absolute mode), d_q, d_e and idx0 as for fa_mx8_decode, on device `gpu`.  ctx may be NULL (then `gpu` is the HIP
 * device).  Every argument is checked before any device call: the dtypes and their pair ((dst, ref) as (in, out)),
 * idx0 + n < 2^64, and for n > 0 null pointers and element alignment of d_ref and d_dst (FA_ERR_ALIGN); with n == 0
 * and valid arguments it returns FA_OK without touching a device.  Any byte phase of d_q and d_e and any element
 * phase of d_ref and d_dst is correct; 16-byte loads and stores are used where the three phases allow a common
 * head.  d_dst must not overlap d_ref.  Async on hip_stream (NULL = the ctx's compute stream of `gpu`, or the null
 * stream). */
int fa_mx8_expand_device(fa_ctx* ctx, int gpu, const int8_t* d_q, const uint8_t* d_e, size_t n, uint64_t idx0,
                         const void* d_ref, fa_dtype ref_dtype, void* d_dst, fa_dtype dst_dtype, void* hip_stream);
/* Lets a part take MX8 receipts (part_id >= 0), or sets the context default for parts defined later (part_id < 0;
 * FA_LITERAL parts ignore it).  A part with it on keeps its device output as the reference g across rounds -- what
 * the last reducing call left there, after a server optimizer or the noise stage the stepped, noisy output: the
 * model the owners were sent -- is never kept host-side (fa_bucket_host_read says 0) and is left non-eager by
 * FA_ACCUMULATE_ON_ARRIVAL.  FA_ERR_ARG, naming the cause: an FA_LITERAL part, an FA_SHARD_CLIENT_RS context (a GPU
 * holding a whole slot does not hold the matching output).  Everything else composes, in any call order: FA_FEDAVG,
 * FA_TRIMMED, every stage, the server optimizers, range shards, range pieces, fa_reduce_parts.  on == 0 frees what it
 * allocated.  Memory: per GPU and client slot a shadow of cnt bytes (cnt the GPU's elements of the bucket; rounded up
 * to 16) plus the scale bytes of the blocks they touch, rounded up to 256, allocated at the part's first fa_submit_mx8 -- about 1/3.9 of an fp32 part's slots
 * on top of them; it keeps a submit fully asynchronous. */
int fa_set_mx8(fa_ctx* ctx, int part_id, int on);
/* An MX8 receipt of client `client_slot`: q (n bytes) and e (fa_mx8_scale_bytes(n) bytes).  flags: FA_HOST_PINNED = q
 * and e are pinned and stay unchanged until fa_finalize* returns, the DMA runs from them; without it they go through
 * the pinned staging chunks and are reusable on return.  FA_MX8_ABSOLUTE = absolute mode (x = d).  Enqueues the H2D of
 * each GPU's bytes of q and of the scale bytes its element range touches, then the expansion into the slot, piece by
 * piece on a part held in pieces, ordered after the part's last reducing call and before the next.  The slot then
 * counts as the client's receipt exactly as after fa_submit (weight, overwriting, fa_bucket_progress).  The reference
 * of a relative submit is the part's device output as the last reducing call left it; FA_ERR_STATE, naming the part,
 * when there is none (the part was never reduced, or fa_set_mx8 was not on when it was, and no
 * fa_mx8_set_reference).  FA_ERR_STATE on a part without fa_set_mx8. */
#define FA_MX8_ABSOLUTE 0x2
int fa_submit_mx8(fa_ctx* ctx, int part_id, int client_slot, const int8_t* q, const uint8_t* e, float weight, int flags);
/* Writes the part's device output on every GPU from host_src (n elements of the out dtype), as if a round had
 * produced it: the reference of the next relative submits (a restarted aggregator; tests).  Waits for the part's
 * pending work.  On a part with the reply stage it also sets `sent`.  FA_ERR_STATE on a part with neither
 * fa_set_mx8 nor fa_set_mx8_reply. */
int fa_mx8_set_reference(fa_ctx* ctx, int part_id, const void* host_src);

/* MX8 replies (the header comment, "MX8 replies"): the new model as block-scaled int8 deltas, encoded on the GPU. */
#define FA_MX8_SCALES_ONLY 0x1  /* write d_e alone: the scales of the blocks from this launch's deltas */
#define FA_MX8_SCALES_GIVEN 0x2 /* read d_e instead of writing it: codes and g' under the given scales */
/* Rules 3-4 on raw device pointers, on device `gpu`: over the n elements of d_new and d_sent (both of dtype
 * new_dtype == sent_dtype), bucket elements idx0 .. idx0 + n - 1, writes d_q (n bytes), d_e (the scale bytes of blocks
 * idx0 >> 5 .. (idx0 + n - 1) >> 5, d_e[0] the first; a block that the launch holds only part of gets the scale of
 * that part) and, unless d_out is NULL, g' into d_out (n elements of the same dtype).  flags: 0 = the fused pass;
 * FA_MX8_SCALES_ONLY = d_e alone is written, d_q and d_out are not touched and may be NULL; FA_MX8_SCALES_GIVEN = d_e
 * is read.  A block cut by launches: scales-only on each part, the byte maximum of the partial scales, scales-given
 * on each part.  Aliasing: d_out may be d_sent or d_new exactly (the same address; both if d_new == d_sent) or
 * overlap neither; d_q and d_e overlap nothing else; any other overlap of d_out is refused with FA_ERR_ARG.  ctx may
 * be NULL (then `gpu` is the HIP device).  Every argument is checked before any device call: the dtypes (equal),
 * the flags (not both), idx0 + n < 2^64, and for n > 0 null pointers and element alignment (FA_ERR_ALIGN); with n == 0
 * and valid arguments it returns FA_OK without touching a device.  Any byte phase of d_q and d_e and any element phase
 * of the others is correct; 16-byte accesses are used where every pointer is 16-byte aligned at the first block
 * boundary.  Async on hip_stream (NULL = the ctx's compute stream of `gpu`, or the null stream). */
int fa_mx8_encode_device(fa_ctx* ctx, int gpu, const void* d_new, fa_dtype new_dtype, const void* d_sent,
                         fa_dtype sent_dtype, size_t n, uint64_t idx0, int8_t* d_q, uint8_t* d_e, void* d_out, int flags,
                         void* hip_stream);
/* Switches the reply stage of a part on or off (part_id >= 0), or sets the context default for parts defined later
 * (part_id < 0; FA_LITERAL parts ignore it).  FA_ERR_ARG on an FA_LITERAL part or an FA_SHARD_CLIENT_RS context.  Like
 * the other stage parts such a part is never kept host-side, FA_ACCUMULATE_ON_ARRIVAL leaves it non-eager, it gets
 * its own launches in fa_reduce_parts, a reducing call needs every client submitted, and fa_reduce_part marks the
 * round reduced.  Switching it on drops `sent` (the next round is a bootstrap); on == 0 frees `sent` and the code
 * buffers.  Memory, allocated at the first reducing call: per GPU its elements once more in the out dtype, one byte
 * per element and the scale bytes. */
int fa_set_mx8_reply(fa_ctx* ctx, int part_id, int on);
/* fa_finalize with the round's codes as the D2H instead of the bucket: q (n bytes) and e (fa_mx8_scale_bytes(n) bytes).
 * flags: FA_HOST_PINNED as in fa_finalize_gather (q and e are pinned, the DMA writes into them).  FA_ERR_STATE,
 * checked before any work and leaving the round intact, when the part has no `sent` (this round is the bootstrap, or
 * the part has no reply stage): the caller then finishes with fa_finalize*. */
int fa_finalize_mx8(fa_ctx* ctx, int part_id, int8_t* q, uint8_t* e, int flags);
/* The codes of the part's last reducing call, as fa_copy_output is for the bucket.  FA_ERR_STATE when that call was
 * a bootstrap (or none was made). */
int fa_copy_mx8(fa_ctx* ctx, int part_id, int8_t* q, uint8_t* e, int flags);
/* *nan_blocks = the E = 255 blocks among the codes of the part's last reducing call (0 after a bootstrap). */
int fa_mx8_reply_stats(fa_ctx* ctx, int part_id, uint64_t* nan_blocks);

/* Compute-node aggregation of an intermediate model part.
 * A compute node keeps one State per client (systemAPI::init_state_vector,
 * systemAPI.cpp:3-15; compute_node.cpp), and the paper (EdgeSys 3) aggregates
 * them, which the reference code never does.  Here every client copy becomes
 * sum_k w_k x_k, in place: the same ordered fp32 FMA chain as FA_FEDAVG,
 * rounded once to the slot dtype and written back to all D slots, so each
 * client continues training from the FedAvg model.  HBM traffic is D*s read +
 * D*s written per element.
 * fa_sync_device: raw device pointers, any D >= 1 (ctx needed only for D > 128).
 * fa_sync_part: the part's own slots on every GPU of the ctx (range shards sync
 * their ranges); h_weights NULL = the weights given to fa_submit.  Both are
 * async on hip_stream (NULL = ctx compute stream). */
int fa_sync_device(fa_ctx* ctx, int gpu, void* const* d_clients, const float* h_weights, int D, size_t n, fa_dtype dt,
                   void* hip_stream);
int fa_sync_part(fa_ctx* ctx, int part_id, const float* h_weights, void* hip_stream);

/* Phased-kernel meetings on HIP device `device` that stopped waiting for the rest of the grid since the
 * process started (each counts one workgroup's bounded wait running out).  Non-zero means the persistent
 * grid was not co-resident -- the GPU was shared with other kernels -- and those launches ran slower;
 * results are unaffected.  Synchronizes with the device. */
int fa_phased_timeouts(int device, uint64_t* count);

/* The phased kernel gives each HIP stream it runs on a counter slot of its own on that device (the first
 * 48 streams; later ones share hashed slots, which costs speed, never results).  A context returns its own
 * streams' slots in fa_destroy; a caller that passed its own stream (fa_reduce_device, fa_sync_device,
 * fa_reduce_part / fa_reduce_parts / fa_sync_part with hip_stream) returns that stream's slot here before it
 * destroys or stops using the stream, so a long-lived process cycling through many streams keeps owned
 * slots.  Launches still in flight on the stream stay correct.  A stream without a slot: FA_OK, no-op. */
int fa_release_stream(int device, void* hip_stream);

/* Literal mode divisor used by fa_reduce_device when ctx == NULL. */
#define FA_DEFAULT_DIVISOR 1000.0f

/* Synthetic input generator on device, identical to oracle/fa_oracle.c:
 * element i = uniform[-1,1) from splitmix64(seed ^ client<<40 ^ (idx0+i)),
 * bf16 and fp16 = round-to-nearest-even of that value. */
int fa_fill_uniform(void* d_dst, size_t n, fa_dtype dt, uint64_t seed, uint32_t client, uint64_t idx0,
                    void* hip_stream);

/* Kernel and layout tuning knobs for benches (every field: 0 = keep the current value). */
typedef struct {
    int block;        /* threads per workgroup: 64, 128 or 256 */
    int max_blocks;   /* grid cap, grid-stride beyond it; -1 = uncapped (one-shot grid) */
    int unroll;       /* clients loaded per FMA group: 4, 8 or 16 */
    int load_policy;  /* client loads: 1 default cache policy, 2 non-temporal */
    int store_policy; /* output stores: 1 plain, 2 nt, 3 sc1 (write-through), 4 sc0 sc1 */
    int slot_skew;    /* bytes between consecutive client slots beyond 4 KiB alignment (multiple of 16);
                         -1 = none, -2 (default) = by slot size: 512 for slots of >= 48 MiB, else 2048;
                         applies to buckets defined afterwards */
    int walk;         /* FedAvg grid walk over a bucket: 1 linear, 2 each XCD's workgroups own one contiguous
                         eighth, 3 the same with the odd eighths walked backwards (one-shot grid only),
                         4 phased: a persistent grid (one workgroup per CU) reduces a phase into LDS and
                         registers, then writes it, so the output never streams beside the inputs,
                         5 (default) phased with a larger register stage (fewer phases; bf16 and
                         fp16 inputs take the form of walk 6), 6 phased with 512-thread workgroups (2 waves per
                         SIMD).  Buckets smaller than one phase (walk 4: 18.9 M, walks 5 and 6:
                         23.1 M elements per GPU on 256 CUs, f32, bf16 or fp16) take walk 2.  The phased
                         kernels always use nt loads and sc1 stores.  With walk 5, a bucket below one
                         phase with >= 16 clients takes one phase sized to it */
    int rs_chunks;    /* FA_SHARD_CLIENT_RS: pieces per round (default 8) */
    int piece_span_kib;  /* range pieces: KiB of a GPU's slots per piece (default 16 GiB); -1 = never cut */
    int piece_split_kib; /* range pieces: a GPU's slots are cut above this many KiB (default 48 GiB); -1 = always */
} fa_tuning;
/* Process defaults: every fa_ctx created afterwards starts from them, and fa_reduce_device /
 * fa_sync_device without a ctx use them. */
int fa_set_tuning(const fa_tuning* t);
int fa_get_tuning(fa_tuning* t);
/* One context's own tuning (buckets defined afterwards take its slot_skew). */
int fa_ctx_set_tuning(fa_ctx* ctx, const fa_tuning* t);
int fa_ctx_get_tuning(fa_ctx* ctx, fa_tuning* t);

/* The rs layout's block-cyclic ownership (FA_SHARD_CLIENT_RS): bucket elements [lo, hi) that GPU `gpu`
 * of n_gpus holds after the reduce-scatter of a bucket of n elements in `chunks` pieces, in the order of
 * its shard (lo_hi: room for 2 * cap values; elements >= n are padding).  Returns the segment count.
 * Pure host arithmetic (no device needed). */
int fa_rs_segments(size_t n, int n_gpus, int chunks, int gpu, size_t* lo_hi, int cap);

#ifdef __cplusplus
}
#endif
#endif /* FEDAVG_FA_H_ */
