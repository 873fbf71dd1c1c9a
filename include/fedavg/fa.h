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
 *   Gram pass (fa_gram_device): the D x D matrix of inner products of D client buckets, optionally against an fp32
 *              reference -- norms, cosines and pairwise distances of updates all come from it.  D <=
 *              FA_DNC_MAX_CLIENTS.
 *              y_k,i is x_k,i widened exactly to fp32 (bf16; fp16 with its subnormals); with a reference y_k,i =
 *              fl32(widen(x_k,i) - ref_i), one IEEE subtract, subnormals kept.  G_ab = sum_i (double)y_a,i *
 *              (double)y_b,i for all a <= b.  Every product is exact in fp64 (24 x 24 significand bits).  The order
 *              and grouping of the fp64 adds is NOT specified, the four-term sum inside a matrix instruction
 *              included; whatever the order |G_ab - exact| <= n * 2^-53 * sum_i |y_a,i y_b,i|.  No floating-point
 *              atomics: for one layout (GPU count, tuning, n, D, pointer phases) the result is the same bits on every
 *              run.  Each pair is computed once and mirrored: the matrix is bit-symmetric.  The diagonal is computed:
 *              G_kk is the squared norm of y_k.  NaN and inf propagate by IEEE rules (0 * inf is NaN); a non-finite
 *              element of client k can only reach row and column k.  On range shards and range pieces the per-shard /
 *              per-piece matrices are added on the host in fp64, in GPU order and then piece order.  Added without a
 *              new FA_ABI_VERSION: fa_gram_device with n == 0 touches no device, writes D * D zeros and answers FA_OK
 *              -- that is how a caller probes for it.
 *   DnC stage (fa_set_dnc): spectral selection of the owners of an FA_FEDAVG part (Divide-and-Conquer: Shejwalkar and
 *              Houmansadr, "Manipulating the Byzantine: Optimizing Model Poisoning Attacks and Defenses for Federated
 *              Learning", NDSS 2021).  Distance rules miss a group of owners that all shift by the same modest
 *              vector; DnC projects the centred buckets on their top singular direction and removes the owners with
 *              the largest projections.  Here the direction comes from the full Gram matrix, not from subsampled
 *              coordinates.  No part-level state and no reference model.  Parameters: drop, the number of owners to
 *              remove (the paper's c f), 0 <= drop, 2 drop < D <= FA_DNC_MAX_CLIENTS; and P, the power iterations,
 *              1 <= P <= FA_DNC_MAX_ITERS.  Rules 2-7 are fa_dnc_select: pure host arithmetic in fp64, every multiply
 *              and add rounded separately (no contraction), sums in client order from +0.  Per round, with weights w_k:
 *              1. Gram.  G is the Gram pass, without a reference (centring removes any common vector), over the
 *                 clients the plain round would reduce.
 *              2. Non-finite buckets.  A client whose G_kk is NaN or +inf is excluded for the round.  R is the rest,
 *                 ascending, r = |R|; by Cauchy-Schwarz every G_ab with a, b in R is finite.  r == 0: the aggregate
 *                 is +0.
 *              3. Centring (unweighted, as in the paper).  rho_a = (sum_{b in R} G_ab) / r, mu = (sum_{a in R}
 *                 rho_a) / r, C_ab = ((G_ab - rho_a) - rho_b) + mu.
 *              4. Start.  a* = the lowest index in R that maximises C_aa.  If C_a*a* is not > 0 (all buckets equal)
 *                 every score is +0 and rules 5-6 are skipped.  Otherwise u_b = C_b,a*.
 *              5. Power iteration, P times.  t_k = sum_{b in R} C_kb u_b, M = max_k |t_k| (NaN if any t_k is).  If M
 *                 is 0 or not finite: stop and keep u.  Otherwise u_k = t_k / M.
 *              6. Scores.  t = C u once more, s_k = t_k t_k: lambda times the squared projection of the centred
 *                 bucket on the top singular direction, which orders the owners as the paper's scores do.
 *              7. Selection.  Excluded clients count against the budget: q = max(0, min(drop - (D - r), r - 1)).  The
 *                 q clients of R with the largest (s_k, k) are removed (ties remove the higher index; a NaN score
 *                 counts as +inf); the rest are selected.  The report: the scores (+inf for an excluded client),
 *                 the flags and their count.
 *              8. Weights and aggregate.  Exactly rules 4 and 5 of the Krum stage: fa_krum_weights, then the chain
 *                 over the selected owners in client order.  With nobody removed it is the plain FA_FEDAVG aggregate
 *                 bit for bit.  It is the part's fp32 aggregate a, as a Krum part's.
 *              A reducing call of such a part enqueues the Gram pass on every GPU, waits for the matrices (one stream
 *              round trip more than a plain round, one more read of the slots), selects on the host and then enqueues
 *              the chain.  Buckets that agree closely leave C with fewer good digits than G; a caller
 *              that holds the last global model can run fa_gram_device against it and fa_dnc_select itself.
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
 *   Top-k receipts (fa_set_topk, fa_submit_topk, fa_topk_expand_device, fa_topk_encode_device, fa_topk_encode,
 *              fa_topk_decode): the other common way to shrink an update.  A client sends only the k elements of
 *              its update x_k - g with the largest magnitude, as (index, value) pairs, and carries the rest over to
 *              its next round (top-k with error feedback): 8 k bytes where fp32 takes 4 n.  As with MX8 receipts a
 *              kernel rebuilds the ordinary slot x = g + d, and everything downstream sees an ordinary receipt.
 *              Format.  A sparse bucket of n elements with k entries is two arrays: idx, k uint32, strictly
 *              ascending, each < n, the element's position in the whole bucket, never within a shard or a piece;
 *              val, k fp32.  A bucket with entries needs n <= 2^32 (FA_ERR_ARG beyond).
 *              Decode (fa_topk_decode): d_i = val_j where i == idx_j, and d_i = +0 everywhere else.
 *              Expansion is decode rule 3 of MX8 receipts, unchanged: x_i = fl32(widen(g_i) + d_i), one IEEE add,
 *              the same add for absent elements, so -0 + +0 is +0; a 16-bit slot stores x_i rounded once more to
 *              nearest-even; without a reference (absolute mode) x_i = d_i, rounded the same way; NaN and inf
 *              propagate, NaN payloads are unspecified; (slot, ref) pairs are the (in, out) pairs below.
 *              Selection (the encoder: fa_topk_encode on given deltas, fa_topk_encode_device on `new` and `sent`
 *              of one dtype), for n elements and k:
 *              1. delta_i = fl32(widen(new_i) - widen(sent_i)), one IEEE subtract, no contraction.
 *              2. key_i = bits(delta_i) & 0x7FFFFFFF: the magnitude order, any NaN above inf, +-0 equal.
 *              3. k' = min(k, n); tau is the k'-th largest key.
 *              4. Selected are all elements with key > tau, plus the lowest-indexed elements with key == tau, until
 *                 exactly k' elements are selected.
 *              5. The entries are written in ascending index order with val_j = delta_i, sign kept, a NaN some quiet
 *                 NaN.  Zeros are selected like any other value when fewer than k' deltas are non-zero.
 *              6. g'_i is the expansion of the selected entries against `sent`, in the same dtype: the model the
 *                 owners hold after the reply.
 *              Every output is specified bit for bit (NaN as NaN) and depends on no grid, tile or run: the kernels
 *              use integer atomics only, whose sums are exact.
 *              Added without a new FA_ABI_VERSION: fa_topk_expand_device and fa_topk_encode_device with n == 0 touch
 *              no device and answer FA_OK -- that is how a caller probes for them.
 *   Low-rank receipts (fa_set_lowrank, fa_submit_lowrank, fa_lowrank_expand_device, fa_lowrank_len, fa_lowrank_decode,
 *              fa_lowrank_check, fa_lowrank_plan_bytes, fa_lowrank_plan_build): the third common way to shrink an update.
 *              The update of a weight matrix M (rows x cols) arrives as P (rows x r) and Q (cols x r) with M ~ P Q^T:
 *              PowerSGD (Vogels et al., NeurIPS 2019), or the factors a federated LoRA owner trains directly, whose
 *              exact aggregate is the weighted sum of the products, not the product of averaged factors.  As with
 *              MX8 and top-k receipts a kernel rebuilds the ordinary slot x = g + d -- here on the matrix unit -- and
 *              everything downstream sees an ordinary receipt; different owners of a round may use different r.
 *              Part table.  A part that takes low-rank receipts has a table of M matrices, fa_lowrank_mat {off, rows,
 *              cols}: rows, cols >= 1; entries ascend by off, do not overlap and satisfy off + rows * cols <= n.
 *              Matrix j is elements off_j + a * cols_j + b of the whole bucket, row-major -- a named_parameters()
 *              tensor of shape [rows, ...] flattened.  Element indices are positions in the whole bucket, never
 *              within a shard or a piece.  `rest` = the elements covered by no matrix (biases, norm layers, matrices
 *              too small to be worth factoring), in ascending order.
 *              Receipt.  One rank r, 1 <= r <= r_max <= FA_LOWRANK_MAX_RANK, and one fp32 array f of
 *              fa_lowrank_len(mats, M, n, r) = r * sum_j (rows_j + cols_j) + |rest| values: for each matrix in table
 *              order P_j (rows_j x r, row-major) then Q_j (cols_j x r, row-major), then the |rest| dense deltas.
 *              Decode (fa_lowrank_decode, pure host arithmetic):
 *              1. For a covered element, S = sum_{t<r} (double)P_j[a,t] * (double)Q_j[b,t].  Every product is exact
 *                 in fp64.  The order and grouping of the fp64 adds is NOT specified, the four-term sum inside a
 *                 matrix instruction included; whatever the order, |S - exact| <= r 2^-53 sum_t |p q|.
 *              2. d = fl32(S), one rounding to nearest-even, subnormals kept.  The host decoder adds in ascending
 *                 t.  Kernel and decoder agree bit for bit wherever the partial sums are exact; elsewhere they
 *                 differ by at most one fp32 ulp, and only when S lies that close to a rounding boundary.
 *              3. For a `rest` element, d is its value.
 *              4. NaN and inf follow IEEE rules (0 * inf is NaN).  A non-finite P_j[a,.] reaches row a only, a
 *                 non-finite Q_j[b,.] column b only.
 *              Expansion is decode rule 3 of MX8 receipts, unchanged: x_i = fl32(widen(g_i) + d_i), one IEEE add; a
 *              16-bit slot stores x_i rounded once more to nearest-even; without a reference (absolute mode)
 *              x_i = d_i, rounded the same way; (slot, ref) pairs are the (in, out) pairs below.
 *              Added without a new FA_ABI_VERSION: fa_lowrank_expand_device with cnt == 0 touches no device and
 *              answers FA_OK -- that is how a caller probes for it.
 *   Rot1 receipts (fa_set_rot1, fa_submit_rot1, fa_rot1_expand_device, fa_rot1_encode_device, fa_rot1_encode,
 *              fa_rot1_decode, fa_rot1_words, fa_rot1_blocks): sign compression under a random rotation (Suresh et al.,
 *              "Distributed Mean Estimation with Limited Communication", ICML 2017; DRIVE, Vargaftik et al., NeurIPS
 *              2021): one bit per element and one fp32 scale per block of 4096, 31.8 times fewer bytes than fp32.  The
 *              rotation, a randomized Walsh-Hadamard transform, gives every coordinate of a block the same scale, which
 *              is what makes one bit useful on heavy-tailed updates; for Gaussian-like updates the NMSE is 1 - 2/pi.
 *              As with the other formats a kernel rebuilds the ordinary slot x = g + d.
 *              Constants.  B = 4096.  Block b is elements [4096 b, 4096 b + 4096) of the whole bucket, never of a
 *              shard or a piece; nb = ceil(n / 4096) (fa_rot1_blocks).
 *              Format.  bits: nb * 128 uint32 words (fa_rot1_words), the bit of element i is bit (i & 31) of word
 *              i >> 5; scale: nb fp32 values; seed: one uint64 chosen by the owner.  In the last block all 4096 bits
 *              are meaningful: they are the transform of the zero-padded block.
 *              Diagonal D.  For element i, with j = i >> 7: Philox4x32-10 as in the noise stage with counter (lo32(j),
 *              hi32(j), 0, 0x524F5431) and key (lo32(seed), hi32(seed)); s_i = bit (i & 31) of output word
 *              (i >> 5) & 3.  "Apply D" flips the IEEE sign bit where s_i is set.
 *              Transform W, on 4096 values: for h = 1, 2, 4, .., 2048 in this order, for every i with (i & h) == 0:
 *              (a, b) = (z_i, z_{i+h}); z_i = fl32(a + b); z_{i+h} = fl32(a - b).  Plain IEEE adds, subnormals kept.
 *              Decode (fa_rot1_decode, and the kernel):
 *              1. u_i = -1.0f where the bit is set, +1.0f elsewhere.
 *              2. v = W(u).  Every intermediate is an integer of magnitude <= 4096, so any order of the stages, or a
 *                 product with +-1 matrices in fp16 x fp16 -> fp32 (H_4096 = H_16 (x) H_16 (x) H_16, and 256 is exact
 *                 in fp16), gives the same bits.
 *              3. d_i = D applied to fl32(v_i * scale_b), one IEEE multiply.  NaN and inf in the scale follow IEEE
 *                 rules (0 * inf is NaN).
 *              4. Elements at or beyond n are dropped.
 *              Expansion is decode rule 3 of MX8 receipts, unchanged: x_i = fl32(widen(g_i) + d_i), one IEEE add; a
 *              16-bit slot stores x_i rounded once more to nearest-even; without a reference (absolute mode)
 *              x_i = d_i, rounded the same way; (slot, ref) pairs are the (in, out) pairs below.
 *              Encode (fa_rot1_encode on given deltas; fa_rot1_encode_device on `new` and `sent` of one dtype), per
 *              block:
 *              1. delta_i = fl32(widen(new_i) - widen(sent_i)), one IEEE subtract.  Elements beyond n are +0.
 *              2. t_i = D applied to delta_i; y = W(t).
 *              3. The bit of i is set iff y_i < 0, an IEEE compare: false for -0 and NaN.
 *              4. A is the sum of (double)|y_i| over a fixed tree: A_i = (double)|y_i|; for h = 1, 2, .., 2048, for
 *                 every i that is a multiple of 2h, A_i += A_{i+h}; A = A_0.
 *              5. If A is NaN or +inf: scale_b = the quiet NaN 0x7FC00000 and all 4096 bits are 0.  Otherwise
 *                 scale_b = (float)(A * 2^-24): the product is exact in fp64 and is rounded once.  This is DRIVE's
 *                 minimum-MSE scale ||Rx||_1 / B folded with the two factors 1/64 of R = H D / 64.
 *              6. g'_i is the expansion of (bits, scale, seed) against `sent`, into the same dtype.
 *              An owner may use another scale, for example the unbiased ||x||^2 / ||Rx||_1 form: any (bits, scale)
 *              is valid decoder input.
 *              Added without a new FA_ABI_VERSION: fa_rot1_expand_device with cnt == 0 and fa_rot1_encode_device with
 *              n == 0 touch no device and answer FA_OK -- that is how a caller probes for them.
 *   Secagg stage (fa_set_secagg, fa_secagg_set_terms, fa_secagg_unmask_device, fa_secagg_mask_host,
 *              fa_secagg_quantize): the server's arithmetic of secure aggregation (Bonawitz et al., "Practical Secure
 *              Aggregation for Privacy-Preserving Machine Learning", CCS 2017).  The slots of an FA_FEDAVG part with
 *              `in` FA_F32 hold uint32 words: an owner's fixed-point update plus its masks modulo 2^32.  A reducing
 *              call sums them, removes the masks the caller names and decodes the sum.  The library knows nothing of
 *              the protocol around it (key agreement, secret sharing, who dropped out).
 *              1. Terms.  A round has T terms, 0 <= T <= FA_SECAGG_MAX_TERMS.  A term is a key of 8 uint32 words, a
 *                 nonce of 3 words and a sign, +1 or -1.  The caller decides which masks to cancel and with which
 *                 sign.
 *              2. Mask word.  Element i is the element's index in the whole bucket, never the index within a shard or
 *                 a piece.  Its mask under a term is word i & 15 of the ChaCha20 block (RFC 8439 2.3: constants, key,
 *                 counter, nonce; 20 rounds; the final addition) with that key and nonce and block counter i >> 4 as
 *                 a uint32.  The word is taken as the state holds it after the final addition: no byte
 *                 serialisation is involved.  idx0 + n <= 2^36 everywhere; more is FA_ERR_ARG.  Known answer: key
 *                 bytes 00 01 .. 1f (words 03020100 07060504 .. 1f1e1d1c), nonce words 09000000 4a000000 00000000,
 *                 counter 1: e4e7f110 15593bd1 1fdd0f50 c47120a3 c7f4d1c7 0368c033 9aaa2204 4e6cd4c3 466482d2 09aa9f07
 *                 05d7c214 a2028bd9 d19c12b5 b94e16de e883d0cb 4e3c50a2 -- as bytes 10 f1 e7 e4 d1 3b 59 15 .., the key
 *                 stream of RFC 8439 2.3.2.
 *              3. Sum.  u_i = sum_k y_{k,i} + sum_t sign_t m_{t,i} modulo 2^32, over the clients the part's plain
 *                 round would reduce.  The order is free: the arithmetic is exact.  Weights are ignored, as for
 *                 FA_TRIMMED: owners put their weight into what they encode.
 *              4. Decode.  a_i = fl32((float)(int32_t)u_i * scale): one conversion to nearest-even and one IEEE fp32
 *                 multiply.  scale is fp32, finite and > 0.
 *              5. Place in the round.  a stands exactly where the chain's result stands: it feeds the noise stage
 *                 and the server optimizer if the part has them, otherwise it is rounded once to the out dtype; MX8
 *                 replies, range shards and range pieces work as for any part.
 *              6. Admission.  The stage belongs to the measure-then-select family: it does not compose with the clip,
 *                 Krum or geomed stage, which need plaintext.  Not with MX8 receipts, not on an FA_SHARD_CLIENT_RS
 *                 context, not as a context default.  Like the other stage parts the part is never kept host-side,
 *                 FA_ACCUMULATE_ON_ARRIVAL leaves it non-eager, and a reducing call needs every client submitted.
 *                 Terms are per round: a reducing call without fa_secagg_set_terms since the last one fails with
 *                 FA_ERR_STATE, so a stale list is never applied; T = 0 is set explicitly.
 *              Owner's side: fa_secagg_quantize makes the fixed-point codes, fa_secagg_mask_host the mask words; both
 *              are pure host arithmetic.  No cryptographic review of the construction is claimed here.  Added without
 *              a new FA_ABI_VERSION: fa_secagg_unmask_device with n == 0 touches no device and answers FA_OK -- that
 *              is how a caller probes for it.
 *   Sign-vote stage (fa_set_sign, fa_submit_sign, fa_copy_sign_planes, fa_sign_vote_device, fa_sign_vote_host,
 *              fa_sign_pack, fa_sign_words, fa_sign_form): signSGD with majority vote (Bernstein et al., "signSGD with
 *              Majority Vote is Communication Efficient and Fault Tolerant", ICLR 2019).  An owner sends one bit per
 *              element, the server counts per element how many owners said "negative", the reply is the sign of the
 *              majority.  The receipts are never expanded: the round reads D / 8 bytes per element of them.
 *              1. Format.  A sign receipt of a bucket of n elements is fa_sign_words(n) = ceil(n / 32) uint32 words;
 *                 the bit of element i is bit i & 31 of word i >> 5, i the element's index in the whole bucket, never
 *                 the index within a shard or a piece.  Bits at or beyond n in the last word are ignored: any value
 *                 there gives the same result.
 *              2. Owner's side (fa_sign_pack, pure host arithmetic).  The bit is set iff delta_i < 0, an IEEE compare:
 *                 clear for -0 and NaN (rot1's encode rule 3).  The padding bits are written as 0.
 *              3. Counts.  c_i is the number of the round's D receipts whose bit i is set, an exact integer, 1 <= D <=
 *                 FA_SIGN_MAX_CLIENTS.  Weights are ignored, as for FA_TRIMMED and the secagg stage.
 *              4. Parameters.  eta: fp32, finite, > 0.  rule: FA_SIGN_MAJORITY or FA_SIGN_MEAN.  margin m, 1 <= m <= D,
 *                 used by the majority rule only (checked where D is known: fa_set_sign, fa_sign_vote_device).
 *              5. Majority.  With s_i = D - 2 c_i: v_i = +1 if s_i >= m, -1 if -s_i >= m, else 0; t_i = +eta, -eta or
 *                 +0.  m = 1 is the paper's vote, a tie on even D giving 0; a larger m is a quorum.
 *              6. Mean.  step = fl32(eta / (float)D), computed once on the host; t_i = fl32((float)s_i * step): one
 *                 exact conversion and one IEEE multiply.
 *              7. Aggregate.  a_i = fl32(widen(g_i) + t_i): one IEEE add, g widened exactly, -0 + +0 is +0; without a
 *                 reference (absolute mode) a_i = t_i.  NaN and inf in g propagate.  a stands exactly where the chain's
 *                 result stands: it feeds the noise stage and the server optimizer if the part has them, otherwise it
 *                 is rounded once to the out dtype; MX8 replies, range shards, range pieces and fa_reduce_parts work as
 *                 for any part.
 *              8. Reference.  g is the part's device output as the last reducing call with the stage left it, exactly
 *                 the reference of MX8 receipts (fa_mx8_set_reference sets it).  A round on a part without a reference
 *                 runs in absolute mode.
 *              9. Vote planes (the compressed reply).  The round optionally leaves two bit planes of fa_sign_words(n)
 *                 words each: neg (the bit is set where v_i = -1) and pos (where v_i = +1), padding bits 0.  An owner
 *                 that holds g and the planes rebuilds the reply bit for bit by rule 7: 2 bits per element where fp32
 *                 takes 32.  The planes exist only under the majority rule on a part with no noise stage and no server
 *                 optimizer (with either the reply is no function of the planes): asking for them otherwise, or
 *                 giving a part with planes one of those stages, is FA_ERR_STATE.
 *              10. Layout independence.  The counts are exact, range shards and pieces are cut at multiples of 64
 *                 elements, so a word never straddles a cut: every output is the same bits for any GPU count, pieces
 *                 or pointer phase.
 *              11. Admission.  Only on an FA_FEDAVG part.  The stage belongs to the measure-then-select family: not
 *                 with the clip, Krum, DnC, geomed or secagg stage (Bulyan needs an FA_TRIMMED part), and not with any of
 *                 the four receipt formats (those setters refuse a sign part in turn).  Not on an FA_SHARD_CLIENT_RS
 *                 context, not as a context default.  Like the other stage parts the part is never kept host-side,
 *                 FA_ACCUMULATE_ON_ARRIVAL leaves it non-eager, and a reducing call needs every client submitted, with
 *                 fa_submit_sign: a dense fa_submit to such a part is FA_ERR_STATE.  Setting the stage on a part drops
 *                 what the round had received so far.
 *              Memory: per GPU and client slot a shadow of ceil(cnt / 32) * 4 bytes, rounded up to 256, and with planes
 *              twice that once more.  The part's dense slots are neither read nor written by a vote round; they stay
 *              allocated (not allocating them is left for later).
 *              Added without a new FA_ABI_VERSION: fa_sign_vote_device with n == 0 touches no device and answers FA_OK
 *              -- that is how a caller probes for it.
 *   Sparse-sum stage (fa_set_sparse_sum, fa_submit_sparse, fa_sparse_sum_device, fa_sparse_sum_host,
 *              fa_sparse_sum_workspace, fa_sparse_sum_form): a round of top-k receipts reduced without expanding them.
 *              sum_c w_c (g + d_c) touches only elements that some owner named, so the round reads the (idx, val) pairs,
 *              8 sum_c k_c bytes, and one dense pass over g, where the expanded route moves 12 D + 4 bytes per element.
 *              Format: the top-k receipt, unchanged (fa_topk_encode and fa_topk_encode_device stay the owner's side): idx
 *              is k strictly ascending uint32, each < n, a position in the whole bucket; val is k fp32.  1 <= D <=
 *              FA_SPARSE_MAX_CLIENTS; 0 <= k_c <= n per client and k_c <= 2^32 - 1 (the kernel's tables count in 32-bit
 *              words: the one receipt that names all 2^32 elements of a bucket of 2^32 is a dense one); n <= 2^32 where
 *              any receipt has entries.
 *              1. Sum.  Per element i: acc = +0; for the clients c in ascending client order that have an entry (i, d):
 *                 acc = fmaf(w_c, d, acc), one fused operation, as in the FA_FEDAVG chain.  Clients without an entry at i
 *                 are skipped, not added as +0.  The one consequence: a partial sum of -0 stays -0, where a chain over
 *                 expanded slots would turn it into +0 at the next client; a partial sum can only be -0 if an exact
 *                 product underflows to zero (a product that is exactly -0 gives -0 + +0 = +0).
 *              2. Aggregate.  a_i = fl32(widen(g_i) + acc_i): one IEEE add, never contracted with rule 1; g widened
 *                 exactly (bf16; fp16 with its subnormals).  The same add is done for elements nobody named, so -0 + +0 =
 *                 +0.  Without a reference (absolute mode) a_i = acc_i.  NaN and inf in val, w or g follow IEEE rules
 *                 (0 * inf is NaN); NaN payloads are unspecified.
 *              3. Weights.  The weights are the owners' shares of the *update*; the reference enters with weight one.  In
 *                 real arithmetic this is the expanded route's result, sum_c w_c (g + d_c), exactly when sum w_c = 1; it
 *                 is not the same bits (the expanded route rounds g + d_c per owner, this one the sum of the updates).
 *                 Any finite or non-finite fp32 weight is taken as given.
 *              4. Place in the round.  a stands exactly where the chain's result stands: it feeds the noise stage and the
 *                 server optimizer if the part has them, otherwise it is rounded once to the out dtype; MX8 replies, range
 *                 shards, range pieces and fa_reduce_parts work as for any part.  The reference g is the part's device
 *                 output as the last reducing call with the stage left it, exactly the reference of MX8 receipts
 *                 (fa_mx8_set_reference sets it).  A round on a part without a reference runs in absolute mode.
 *              5. Layout independence.  Every element's arithmetic is a fixed sequence that depends on no tile, grid, shard
 *                 or piece: every output is the same bits for any GPU count, pieces, pointer phase or kernel form.
 *              6. Admission.  Only on an FA_FEDAVG part.  The stage belongs to the measure-then-select family: not with
 *                 the clip, Krum, DnC, geomed, secagg or sign stage (Bulyan needs an FA_TRIMMED part), and not with any of
 *                 the four receipt formats (those setters refuse a sparse-sum part in turn).  Not on an
 *                 FA_SHARD_CLIENT_RS context, not as a context default.  Like the other stage parts the part is never kept
 *                 host-side, FA_ACCUMULATE_ON_ARRIVAL leaves it non-eager, and a reducing call needs every client
 *                 submitted, with fa_submit_sparse: a dense fa_submit to such a part is FA_ERR_STATE.  Setting the stage
 *                 on a part drops what the round had received so far.
 *              Memory: per GPU and client slot a shadow of min(k_max, cnt) * 8 bytes, rounded up to 256, and per GPU one
 *              workspace of fa_sparse_sum_workspace(cnt, D) bytes.  The part's dense slots are neither read nor written
 *              by such a round; they stay allocated (not allocating them is left for later).
 *              Added without a new FA_ABI_VERSION: fa_sparse_sum_device with n == 0 touches no device and answers FA_OK
 *              -- that is how a caller probes for it.
 *   MX8-sum stage (fa_set_mx8_sum, fa_submit_mx8_sum, fa_mx8_sum_device, fa_mx8_sum_host, fa_mx8_sum_form): a round of
 *              MX8 receipts reduced without expanding them.  With the weights as shares of the update, sum_c w_c (g + d_c)
 *              is g + sum_c w_c d_c, so the round reads the D code streams as they are, one byte per owner and element and
 *              one scale byte per owner and 32 elements, reads g once and writes the output once: 1.03 D + 8 bytes per
 *              element with fp32 g and output, where fa_submit_mx8 and the chain move about 13 D + 4.
 *              Format: the MX8 receipt, unchanged (fa_mx8_encode and fa_mx8_encode_device stay the owner's side): q is n
 *              int8, e is ceil(n / 32) bytes, the block of element i is i >> 5 of the whole bucket.  1 <= D <=
 *              FA_MX8_SUM_MAX_CLIENTS.
 *              1. Decode.  d_c,i is decode rules 1-2 of MX8 receipts, unchanged: a quiet NaN for E = 255, else
 *                 fl32((float)q * 2^(E - 133)), one IEEE multiply, subnormal scales kept; -128 at E = 254 gives -inf.
 *              2. Sum.  Per element i: acc = +0; for every client c in ascending order acc = fmaf(w_c, d_c,i, acc), one
 *                 fused operation, as in the FA_FEDAVG chain.  Every client has a value at every element: nobody is
 *                 skipped.  The scale is not folded into the weight (w_c * 2^(E - 133) can round where q * 2^(E - 133)
 *                 cannot): the multiply of rule 1 is done, then the fma.
 *              3. Aggregate.  a_i = fl32(widen(g_i) + acc_i): one IEEE add, never contracted with rule 2; g widened
 *                 exactly (bf16; fp16 with its subnormals).  Without a reference (absolute mode) a_i = acc_i.  NaN and inf
 *                 in d, w or g follow IEEE rules (0 * NaN is NaN); NaN payloads are unspecified.
 *              4. Weights, place in the round, reference, layout independence, admission: what rules 3-6 of the sparse-sum
 *                 stage say, with fa_set_mx8_sum and fa_submit_mx8_sum in place of fa_set_sparse_sum and fa_submit_sparse.
 *                 The weights are the owners' shares of the *update* and g enters with weight one; any fp32 weight is taken
 *                 as given.  a stands exactly where the chain's result stands: it feeds the noise stage and the server
 *                 optimizer if the part has them, otherwise it is rounded once to the out dtype; MX8 replies, range shards,
 *                 range pieces and fa_reduce_parts work as for any part.  The reference g is the part's device output as
 *                 the last reducing call with the stage left it (fa_mx8_set_reference sets it); a round on a part without
 *                 a reference runs in absolute mode.  Every element's arithmetic is a fixed sequence that depends on no
 *                 tile, grid, shard or piece: the same bits for any GPU count, pieces, pointer phase or kernel form.  Only
 *                 on an FA_FEDAVG part; a member of the measure-then-select family: not with the clip, Krum, DnC, geomed,
 *                 secagg, sign or sparse-sum stage, and not with any of the four receipt formats (those setters refuse an
 *                 MX8-sum part in turn).  Not on an FA_SHARD_CLIENT_RS context, not as a context default.  The part is never
 *                 kept host-side, FA_ACCUMULATE_ON_ARRIVAL leaves it non-eager, and a reducing call needs every client
 *                 submitted, with fa_submit_mx8_sum: a dense fa_submit to such a part is FA_ERR_STATE.  Setting the stage on
 *                 a part drops what the round had received so far.
 *              5. One identity.  In absolute mode with an f32 output the result is bit for bit what the same receipts give
 *                 through fa_set_mx8 with FA_MX8_ABSOLUTE into f32 slots and the chain: the same fma chain over the same d.
 *                 In relative mode the bits differ: the expanded route rounds g + d_c per owner.
 *              Memory: per GPU and client slot one shadow in the MX8 shadow layout (cnt bytes of q rounded up to 16, then
 *              the scale bytes of the blocks the range touches, rounded up to 256), allocated at the part's first submit.
 *              The part's dense slots are neither read nor written by such a round; they stay allocated.
 *              Added without a new FA_ABI_VERSION: fa_mx8_sum_device with n == 0 touches no device and answers FA_OK --
 *              that is how a caller probes for it.
 *   Low-rank-sum stage (fa_set_lowrank_sum, fa_submit_lowrank_sum, fa_lowrank_sum_device, fa_lowrank_sum_host): a round
 *              of low-rank receipts reduced without expanding them.  The weighted sum of the owners' products is itself
 *              one matrix product, sum_c w_c P_c Q_c^T = [w_1 P_1 | ... | w_D P_D] [Q_1 | ... | Q_D]^T -- the "stacking"
 *              form of exact federated LoRA aggregation -- so the round reads g once and writes the aggregate once: 8 bytes
 *              per element with fp32 g and output, where fa_submit_lowrank and the chain move about 12 D + 4.  It runs the
 *              fp64 multiply-adds the D expansions run together, and rounds once where they round D + 1 times.
 *              Format: the low-rank receipt, unchanged: the part's table of fa_lowrank_mat, one rank per owner, 1 <= r_c <=
 *              r_max <= FA_LOWRANK_MAX_RANK, and f_c of fa_lowrank_len(.., r_c) floats.  Owners may differ in rank.  1 <= D
 *              <= FA_LOWRANK_SUM_MAX_CLIENTS.
 *              1. Weighted factor.  p'_c[a,t] = fl32(w_c * P_c[a,t]), one IEEE fp32 multiply, subnormals kept.  The weight
 *                 goes onto P, never onto Q, and it is not applied in fp64: w P Q would then be no exact fp64 product.
 *              2. Stacked sum, covered elements.  S = sum_c sum_{t < r_c} (double)p'_c[a,t] * (double)Q_c[b,t].  Every
 *                 product is exact in fp64.  The order and grouping of the fp64 adds is NOT specified, the four-term sum
 *                 inside a matrix instruction included; whatever the order, |S - exact| <= K 2^-53 sum |p' q| with K =
 *                 sum_c r_c.  acc = fl32(S), one rounding to nearest-even.  The host twin adds in ascending (c, t).  Kernel
 *                 and twin agree bit for bit wherever the partial sums are exact; elsewhere they differ by at most one fp32
 *                 ulp, and only when S lies that close to a rounding boundary (low-rank receipts, rule 2).
 *              3. Rest elements.  acc = +0; for every client c in ascending order acc = fmaf(w_c, d_c,i, acc), one fused
 *                 operation: the chain of the other sum stages, bit-specified.
 *              4. Aggregate.  a_i = fl32(widen(g_i) + acc_i): one IEEE add, never contracted; g widened exactly.  Without a
 *                 reference (absolute mode) a_i = acc_i.  NaN and inf follow IEEE rules: a non-finite P_c[a,.] reaches row
 *                 a only, a non-finite Q_c[b,.] column b only, and w_c = 0 with an inf in P_c gives NaN.
 *              5. Weights, place in the round, reference, layout independence, admission: what rules 3-6 of the sparse-sum
 *                 stage say, with fa_set_lowrank_sum and fa_submit_lowrank_sum in place of fa_set_sparse_sum and
 *                 fa_submit_sparse (layout independence within rule 2: a covered element's fp64 adds may be grouped by
 *                 tile).  Only on an FA_FEDAVG part; a member of the measure-then-select family: not with the clip, Krum,
 *                 DnC, geomed, secagg, sign, sparse-sum or MX8-sum stage, and not with any of the four receipt formats
 *                 (those setters refuse a low-rank-sum part in turn).  Not on an FA_SHARD_CLIENT_RS context, not as a
 *                 context default.  A dense fa_submit to such a part is FA_ERR_STATE.  Setting the stage on a part drops
 *                 what the round had received so far.
 *                 Unlike MX8-sum rule 5 there is NO bit identity with the expanded route, not even in absolute mode: that
 *                 route rounds each owner's product to fp32 and then chains them, this one rounds the sum once.  It is at
 *                 least as accurate.
 *              Memory: per GPU and client slot a shadow of fa_lowrank_len(.., r_max) floats, rounded up to 256 bytes,
 *              allocated at the part's first fa_submit_lowrank_sum, and per GPU the plans of its pieces.  The part's dense
 *              slots are neither read nor written by such a round; they stay allocated.
 *              Added without a new FA_ABI_VERSION: fa_lowrank_sum_device with cnt == 0 touches no device and answers
 *              FA_OK -- that is how a caller probes for it.
 *   Rot1-sum stage (fa_set_rot1_sum, fa_submit_rot1_sum, fa_rot1_sum_device, fa_rot1_sum_host): a round of rot1 receipts
 *              reduced in the rotated domain, without expanding them.  The transform is linear: with H the +-1 transform W,
 *              D_s the sign diagonal of seed s and u_c the +-1 vector of owner c's bits, for the owners that share s
 *                  sum_c w_c D_s(scale_c H u_c) = D_s H(sum_c (w_c scale_c) u_c),
 *              so the round adds the owners' signed scalars per rotated coordinate, D adds and no multiply, runs one
 *              real-valued transform per block and seed, and adds g once: D / 8 + 8 bytes per element with fp32 g and
 *              output, where fa_submit_rot1 and the chain move about 12 D + 4.
 *              Format: the rot1 receipt, unchanged (bits, scale, seed; fa_rot1_encode and fa_rot1_encode_device stay the
 *              owner's side).  1 <= D <= FA_ROT1_SUM_MAX_CLIENTS.  Block b is elements [4096 b, 4096 b + 4096) of the
 *              whole bucket, never of a shard or a piece.
 *              0. Seed groups.  The owners of a round are grouped by seed; the groups are ordered by their lowest client
 *                 slot, the owners of a group by ascending slot.  One seed for all (the server announced the rotation) is
 *                 one group, the fast case; a seed per owner (DRIVE's independent rotations, whose quantisation errors
 *                 average out better) is D groups: still no dense slot moves, but every owner pays a transform.  Both
 *                 are valid, the choice is the caller's; DESIGN.md 8s says what each costs.
 *              1. Scalar.  Per block b and owner c: t_c = fl32(w_c * scale_c,b), one IEEE multiply.
 *              2. Rotated-domain chain.  Per group G and position j of the block (all 4096, the zero-padded tail of the
 *                 last block included): z_j = +0; then for the owners c of G in order z_j = fl32(z_j + s), s being t_c
 *                 with its IEEE sign bit flipped where bit j of owner c is set.  Plain adds, never contracted.
 *              3. Transform.  v = W(z), exactly "Transform W" of Rot1 receipts: h = 1, 2, .., 2048 in that order,
 *                 fl32(a + b) and fl32(a - b), subnormals kept.
 *              4. Diagonal.  d_G,i is v_i with its sign flipped where the group's seed says so ("Diagonal D").
 *              5. Sum over groups.  acc_i = +0; then for the groups in order acc_i = fl32(acc_i + d_G,i).
 *              6. Aggregate.  a_i = fl32(widen(g_i) + acc_i), one IEEE add; without a reference (absolute mode) a_i =
 *                 acc_i.  Elements at or beyond n are dropped.  NaN and inf in scale, w or g follow IEEE rules: a NaN
 *                 scale, which the encoder emits for a non-finite block, makes that block NaN and no other.  NaN payloads
 *                 are unspecified.
 *              7. Weights, place in the round, reference, layout independence, admission: what rules 3-6 of the sparse-sum
 *                 stage say, with fa_set_rot1_sum and fa_submit_rot1_sum in place of fa_set_sparse_sum and
 *                 fa_submit_sparse.  The weights are the owners' shares of the *update* and g enters with weight one; a
 *                 stands exactly where the chain's result stands: noise, server optimizers, MX8 replies, range shards,
 *                 range pieces and fa_reduce_parts follow unchanged.  Only on an FA_FEDAVG part; a member of the
 *                 measure-then-select family: not with the clip, Krum, DnC, geomed, secagg, sign, sparse-sum, MX8-sum or
 *                 low-rank-sum stage, and not with any of the four receipt formats (those setters refuse a rot1-sum part
 *                 in turn).  Not on an FA_SHARD_CLIENT_RS context, not as a context default.  A dense fa_submit to such a
 *                 part is FA_ERR_STATE.  Setting the stage on a part drops what the round had received so far.  Shards
 *                 and pieces are cut at multiples of 64, not 4096: as in fa_rot1_expand_device a block that a range holds
 *                 part of is reduced whole and stored only inside the range.  A block's arithmetic never depends on the
 *                 range: the same bits for any GPU count, pieces, pointer phase or kernel form.
 *              8. Identities.  There is NO bit identity with the expanded route in general: that route rounds v * scale
 *                 once per owner, this one rounds inside the transform.  There is one wherever every partial sum is exact
 *                 in fp32: one owner, w = 1 and a scale of at most 12 significant bits give fl32(+0 + d_i) with d_i
 *                 fa_rot1_decode's value -- its bits, except that rule 5 starts from +0, so the decoder's -0 comes out
 *                 +0.  The error against the exact sum is bounded in DESIGN.md 8s.
 *              Memory: per GPU and client slot one shadow in the rot1 shadow layout (516 bytes per block its range touches,
 *              rounded up to 256), allocated at the part's first fa_submit_rot1_sum.  The part's dense slots are neither
 *              read nor written by such a round; they stay allocated.
 *              Added without a new FA_ABI_VERSION: fa_rot1_sum_device with cnt == 0 touches no device and answers FA_OK --
 *              that is how a caller probes for it.
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
/* Most clients of a part with the DnC stage, and of fa_gram_device (more: FA_ERR_ARG); most power iterations. */
#define FA_DNC_MAX_CLIENTS 128
#define FA_DNC_MAX_ITERS 1024
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

/* The Gram pass on raw device pointers (the header comment, "Gram pass"): h_gram (D * D doubles, row-major) = the
 * matrix G of the D client buckets (n elements of `in`) on device `gpu`, against d_ref (n fp32) unless it is NULL, 1
 * <= D <= FA_DNC_MAX_CLIENTS.  ctx may be NULL (then `gpu` is the HIP device).  Every argument is checked before any
 * device call: D, the dtype, h_gram, and for n > 0 null pointers and element alignment (FA_ERR_ALIGN); with n == 0
 * and valid arguments it touches no device, writes D * D zeros and answers FA_OK.  Otherwise it enqueues on
 * hip_stream (NULL = the ctx's compute stream of `gpu`, or the null stream), waits for it and returns the matrix. */
int fa_gram_device(fa_ctx* ctx, int gpu, const void* const* d_clients, int D, size_t n, fa_dtype in, const float* d_ref,
                   double* h_gram, void* hip_stream);
/* DnC stage: spectral selection of an FA_FEDAVG part's owners (the header comment, "DnC stage").  Gives a part the
 * stage with parameters drop and iters (part_id >= 0; calling again changes them), or sets the context default that
 * FA_FEDAVG parts defined later take (part_id < 0; checked against D when such a part is defined, where a misfit
 * makes fa_bucket_define fail).  iters == 0 removes the stage.  FA_ERR_ARG, naming the cause: drop < 0, iters outside
 * 0..FA_DNC_MAX_ITERS, a drop that does not fit the part's D (2 drop < D), D > FA_DNC_MAX_CLIENTS, an FA_LITERAL or
 * FA_TRIMMED part, an FA_SHARD_CLIENT_RS context, a part (or context default) that has the clip, Krum, geomed or secagg
 * stage -- and those setters on a DnC part: they do not compose.  The noise stage, the server optimizers, MX8 receipts
 * and replies compose, in either call order; range shards and range pieces work.  As a Krum part it is never kept
 * host-side, never eager, gets its own launches in fa_reduce_parts, and a reducing call needs every client submitted
 * and waits on the host for the Gram pass before it enqueues the chain.  The stage keeps no state across rounds. */
int fa_set_dnc(fa_ctx* ctx, int part_id, int drop, int iters);
/* What the part's last reducing call did: gram = the D x D matrix G (row-major), scores[k] = s_k (+inf: excluded),
 * selected[k] = 0 / 1, *n_selected = how many are selected.  Any pointer may be NULL.  FA_ERR_STATE on a part without
 * the stage or never reduced with it. */
int fa_dnc_get_round(fa_ctx* ctx, int part_id, double* gram, double* scores, int* selected, int* n_selected);
/* Rules 2-7 of the stage, pure host arithmetic, usable without a device: the scores and the selection flags (D
 * entries each, either may be NULL) of the D x D row-major matrix gram under drop and iters.  FA_ERR_ARG for a null
 * gram, D < 1 or D > FA_DNC_MAX_CLIENTS, drop < 0 or 2 drop >= D, iters outside 1..FA_DNC_MAX_ITERS.  The weights of the
 * round are fa_krum_weights of the flags. */
int fa_dnc_select(const double* gram, int D, int drop, int iters, double* scores, int* selected, int* n_selected);

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
 * pending work.  On a part with the reply stage it also sets `sent`.  FA_ERR_STATE on a part with none of
 * fa_set_mx8, fa_set_topk, fa_set_lowrank, fa_set_rot1 and fa_set_mx8_reply. */
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

/* Top-k receipts (the header comment, "Top-k receipts"): the k largest elements of an update, expanded and selected
 * on the GPU. */
/* Rules 2-5 on the n given deltas, pure host arithmetic, usable without a device: idx and val get min(k, n) entries,
 * *k_out (nullable) = min(k, n). */
int fa_topk_encode(const float* delta, size_t n, size_t k, uint32_t* idx, float* val, size_t* k_out);
/* The decoder, pure host arithmetic: d[i] = the delta of bucket element idx0 + i over n elements; entries outside
 * [idx0, idx0 + n) are skipped.  FA_ERR_ARG, naming the entry, if idx is not strictly ascending. */
int fa_topk_decode(const uint32_t* idx, const float* val, size_t k, uint64_t idx0, size_t n, float* d);
/* The expansion on raw device pointers, on device `gpu`: d_dst[i] (n of dst_dtype) = fl(widen(d_ref[i]) + d_i), or d_i
 * with d_ref NULL (absolute mode), over bucket elements idx0 .. idx0 + n - 1.  d_idx and d_val are the k entries to
 * look at, the whole bucket's or a range's; entries outside the range are ignored; k == 0 is a plain convert/copy of
 * the reference, or zeros.  Ascending order is the caller's obligation here: with unsorted or duplicate indices the
 * values written are unspecified, but nothing is written outside d_dst[0, n) -- every entry is range-checked where
 * it is applied.  ctx may be NULL (then `gpu` is the HIP device).  Every argument is checked before any device call:
 * the dtypes and their pair ((dst, ref) as (in, out)), idx0 + n < 2^64, and for n > 0 null pointers and element
 * alignment (FA_ERR_ALIGN); with n == 0 and valid arguments it returns FA_OK without touching a device.  Any element
 * phase of d_ref and d_dst is correct; 16-byte loads and stores are used where the two phases allow a common head.
 * d_dst must not overlap d_ref.  Async on hip_stream (NULL = the ctx's compute stream of `gpu`, or the null stream). */
int fa_topk_expand_device(fa_ctx* ctx, int gpu, const uint32_t* d_idx, const float* d_val, size_t k, size_t n,
                          uint64_t idx0, const void* d_ref, fa_dtype ref_dtype, void* d_dst, fa_dtype dst_dtype,
                          void* hip_stream);
/* The bytes of fa_topk_encode_device's scratch for n elements: the histogram and two counters per tile of 4096
 * elements -- never O(n). */
size_t fa_topk_encode_workspace(size_t n);
/* Rules 1-6 on raw device pointers, on device `gpu`: over the n elements of d_new and d_sent (one dtype), d_idx and
 * d_val get min(k, n) entries and, unless d_out is NULL, d_out gets g' (n elements of the same dtype).  d_out may be
 * d_sent or d_new exactly or overlap neither (FA_ERR_ARG otherwise).  d_work: fa_topk_encode_workspace(n) bytes,
 * 16-byte aligned, not initialised by the caller.  All launches are enqueued without a host round trip: the threshold,
 * the count of ties and the tile offsets travel through d_work, which a later call on the same stream may reuse.  The
 * checks, ctx == NULL, the n == 0 probe and the stream are fa_topk_expand_device's. */
int fa_topk_encode_device(fa_ctx* ctx, int gpu, const void* d_new, fa_dtype new_dtype, const void* d_sent,
                          fa_dtype sent_dtype, size_t n, size_t k, uint32_t* d_idx, float* d_val, void* d_out,
                          void* d_work, void* hip_stream);
/* Lets a part take top-k receipts of at most k_max entries (part_id >= 0; 0 = off), or sets the context default for
 * parts defined later (part_id < 0).  It is the stage of fa_set_mx8 with a second format: admission, the reference,
 * the refusals (FA_LITERAL, FA_SHARD_CLIENT_RS, a secagg part) and the call ordering are fa_set_mx8's, the part is
 * never kept host-side and FA_ACCUMULATE_ON_ARRIVAL leaves it non-eager.  A part may have both, and different owners
 * may send different formats.  Memory: per GPU and client slot a shadow of min(k_max, cnt) * 8 bytes, rounded up to
 * 256, allocated at the part's first fa_submit_topk; a changed k_max frees it. */
int fa_set_topk(fa_ctx* ctx, int part_id, size_t k_max);
/* A top-k receipt of client `client_slot`: k <= k_max entries.  flags: FA_HOST_PINNED as for fa_submit_mx8 (idx and val
 * stay unchanged until fa_finalize* returns); FA_TOPK_ABSOLUTE = absolute mode (x = d).  Checks on the host, before
 * anything is enqueued, that idx is strictly ascending and < n (FA_ERR_ARG naming the first bad entry; the round stays
 * as it was), splits the entries into each GPU's element range and each piece's, enqueues the H2D of each sub-array
 * and the expansion with that range's idx0, ordered after the part's last reducing call and before the next.  The slot
 * then counts as the client's receipt exactly as after fa_submit.  The reference and its FA_ERR_STATE are
 * fa_submit_mx8's; FA_ERR_STATE on a part without fa_set_topk. */
#define FA_TOPK_ABSOLUTE 0x2
int fa_submit_topk(fa_ctx* ctx, int part_id, int client_slot, const uint32_t* idx, const float* val, size_t k,
                   float weight, int flags);

/* Low-rank receipts (the header comment, "Low-rank receipts"): factor pairs expanded on the GPU by fp64 MFMA. */
#define FA_LOWRANK_MAX_RANK 64
typedef struct {
    uint64_t off;  /* the matrix's first element in the whole bucket */
    uint32_t rows; /* >= 1 */
    uint32_t cols; /* >= 1; element (a, b) is off + a * cols + b */
} fa_lowrank_mat;
/* The table rules against a bucket of n elements, pure host arithmetic: FA_ERR_ARG naming the first bad entry (no rows
 * or columns, descending, overlapping, beyond n).  Every function below that takes a table checks it so. */
int fa_lowrank_check(const fa_lowrank_mat* mats, size_t M, size_t n);
/* The fp32 values of a receipt of rank r: r * sum_j (rows_j + cols_j) + |rest|.  0 with fa_last_error set for a bad
 * table or a rank outside 1 .. FA_LOWRANK_MAX_RANK. */
size_t fa_lowrank_len(const fa_lowrank_mat* mats, size_t M, size_t n, int r);
/* The decoder, pure host arithmetic: d[i] = the delta of bucket element idx0 + i over cnt elements (idx0 + cnt <= n),
 * the fp64 sums added in ascending t. */
int fa_lowrank_decode(const fa_lowrank_mat* mats, size_t M, size_t n, const float* f, int r, uint64_t idx0, size_t cnt,
                      float* d);
/* The plan of one launch over bucket elements [idx0, idx0 + cnt), host-only: the output tiles of every matrix the
 * range meets and the rest elements against their offsets in f, an opaque blob that the caller puts into device
 * memory (8-byte aligned).  It does not depend on r.  fa_lowrank_plan_bytes: its size, a multiple of 32 (0 with
 * fa_last_error set for a bad table or range); fa_lowrank_plan_build writes it, plan_bytes being exactly that size. */
size_t fa_lowrank_plan_bytes(const fa_lowrank_mat* mats, size_t M, size_t n, uint64_t idx0, size_t cnt);
int fa_lowrank_plan_build(const fa_lowrank_mat* mats, size_t M, size_t n, uint64_t idx0, size_t cnt, void* plan,
                          size_t plan_bytes);
/* The expansion on raw device pointers, on device `gpu`: d_dst[i] (cnt of dst_dtype) = fl(widen(d_ref[i]) + d_i), or d_i
 * with d_ref NULL (absolute mode), over bucket elements idx0 .. idx0 + cnt - 1, from the whole receipt d_f (rank r) and
 * the plan built for exactly this range (d_plan, plan_bytes); a plan of another range leaves d_dst untouched.  One
 * launch: a workgroup per output tile and per chunk of rest elements; every store is checked against the tile, the
 * matrix and the range, so nothing is written outside d_dst[0, cnt).  ctx may be NULL (then `gpu` is the HIP device).
 * Every argument is checked before any device call: the dtypes and their pair ((dst, ref) as (in, out)), idx0 + cnt <
 * 2^64, and for cnt > 0 the rank, the plan size, null pointers, alignment (FA_ERR_ALIGN: d_plan 8 bytes, d_f 4, d_ref
 * and d_dst their element) and that d_dst does not overlap d_ref (FA_ERR_ARG); with cnt == 0 and valid arguments it
 * returns FA_OK without touching a device.  Any element phase of d_ref and d_dst is correct; 16-byte loads and stores
 * are used where the two phases agree.  Async on hip_stream (NULL = the ctx's compute stream of `gpu`, or the null
 * stream). */
int fa_lowrank_expand_device(fa_ctx* ctx, int gpu, const void* d_plan, size_t plan_bytes, const float* d_f, int r,
                             uint64_t idx0, size_t cnt, const void* d_ref, fa_dtype ref_dtype, void* d_dst,
                             fa_dtype dst_dtype, void* hip_stream);
/* Lets a part take low-rank receipts of rank at most r_max over the table mats[0, M) (copied); M == 0 switches them
 * off.  part_id < 0 is refused (FA_ERR_ARG): a table belongs to one part's layout, there is no context default.  It is
 * the stage of fa_set_mx8 with a third format: admission, the reference, the refusals (FA_LITERAL, FA_SHARD_CLIENT_RS, a
 * secagg part) and the call ordering are fa_set_mx8's, the part is never kept host-side and FA_ACCUMULATE_ON_ARRIVAL
 * leaves it non-eager.  A part may take all three formats, and different owners may send different ones.  The plans of
 * every GPU's range and piece are built and uploaded here.  Memory: per GPU and client slot a shadow of
 * fa_lowrank_len(.., r_max) floats, rounded up to 256 bytes, allocated at the part's first fa_submit_lowrank; a changed
 * table or r_max frees it. */
int fa_set_lowrank(fa_ctx* ctx, int part_id, const fa_lowrank_mat* mats, size_t M, int r_max);
/* A low-rank receipt of client `client_slot`: rank r <= r_max and f, len values, where len must be
 * fa_lowrank_len(.., r) (FA_ERR_ARG otherwise, as for r; the round stays as it was).  flags:
 * FA_HOST_PINNED as for fa_submit_mx8 (f stays unchanged until fa_finalize* returns); FA_LOWRANK_ABSOLUTE = absolute
 * mode (x = d).  Copies f to every GPU that holds part of the slot -- a shard needs the rows and columns of every tile
 * it touches, and factors are small -- and enqueues the expansion per GPU and per piece with that range's plan, ordered
 * after the part's last reducing call and before the next.  The slot then counts as the client's receipt exactly as
 * after fa_submit.  The reference and its FA_ERR_STATE are fa_submit_mx8's; FA_ERR_STATE on a part without
 * fa_set_lowrank. */
#define FA_LOWRANK_ABSOLUTE 0x2
int fa_submit_lowrank(fa_ctx* ctx, int part_id, int client_slot, const float* f, size_t len, int r, float weight,
                      int flags);

/* Low-rank-sum stage (the header comment, "Low-rank-sum stage"): a round of low-rank receipts reduced as one stacked
 * product on the fp64 matrix unit, without expanding them. */
#define FA_LOWRANK_SUM_MAX_CLIENTS 128
/* Rules 1-4 on the host, usable without a device: out[i] (fp32, cnt elements) is the aggregate of bucket element idx0 + i
 * from the whole receipts f[c] of rank r[c] under w[c], c < D, and ref (fp32, cnt elements, NULL = absolute mode); the
 * fp64 sums added in ascending (c, t).  FA_ERR_ARG for a bad table, D, rank or range and for null pointers. */
int fa_lowrank_sum_host(const fa_lowrank_mat* mats, size_t M, size_t n, const float* const* f, const int* r, const float* w,
                        int D, uint64_t idx0, size_t cnt, const float* ref, float* out);
/* Rules 1-4 on raw device pointers, on device `gpu`: d_out[i] (cnt of out_dtype, one rounding) over bucket elements idx0 ..
 * idx0 + cnt - 1 from d_ref (cnt of ref_dtype, NULL = absolute mode), the whole receipts d_f[c] (device memory, rank r[c])
 * under w[c], and the plan built for exactly this range (d_plan, plan_bytes: fa_lowrank_plan_build; it does not depend on
 * a rank, and a plan of another range leaves d_out untouched).  The arrays d_f, r and w themselves are host memory and are
 * read before the call returns.  One launch: a workgroup per plan record; every store is checked against the tile, the
 * matrix and the range, so nothing is written outside d_out[0, cnt).  ctx may be NULL (then `gpu` is the HIP device).
 * Every argument is checked before any device call: the dtypes and their pair, 1 <= D <= FA_LOWRANK_SUM_MAX_CLIENTS, idx0 +
 * cnt < 2^64, and for cnt > 0 every rank, the plan size, null pointers, alignment (FA_ERR_ALIGN: d_plan 8 bytes, every
 * d_f[c] 4, d_ref and d_out their element) and that d_out does not overlap d_ref (FA_ERR_ARG); with cnt == 0 and valid
 * arguments it returns FA_OK without touching a device.  Any element phase of d_ref and d_out is correct; 16-byte loads
 * and stores are used where the two phases agree.  Async on hip_stream (NULL = the ctx's compute stream of `gpu`, or the
 * null stream). */
int fa_lowrank_sum_device(fa_ctx* ctx, int gpu, const void* d_plan, size_t plan_bytes, const float* const* d_f, const int* r,
                          const float* w, int D, uint64_t idx0, size_t cnt, const void* d_ref, fa_dtype ref_dtype, void* d_out,
                          fa_dtype out_dtype, void* hip_stream);
/* Gives a part the stage (part_id >= 0, M > 0) over the table mats[0, M) (copied) for receipts of rank at most r_max: its
 * rounds take low-rank receipts with fa_submit_lowrank_sum and reduce them by rules 1-4 against the part's last output;
 * the round under way is dropped, and the plans of every GPU's range and piece are built and uploaded.  Again with the
 * same table and r_max: nothing; with another: the shadows and what the round received go, the reference stays.  M == 0
 * removes the stage and frees what it allocated.  FA_ERR_ARG, naming the cause: a bad table, r_max outside 1 ..
 * FA_LOWRANK_MAX_RANK, D > FA_LOWRANK_SUM_MAX_CLIENTS, part_id < 0 (no context default), a part whose mode is not
 * FA_FEDAVG, a part with a clip, Krum, DnC, geomed, secagg, sign, sparse-sum, MX8-sum or receipt stage (those setters
 * refuse a low-rank-sum part in turn), an FA_SHARD_CLIENT_RS context.  In DESIGN.md 8r the stage takes 0.23 - 0.79 of the
 * expanded route's device time at r = 4 and 16 (D = 8, 32, 64; 64 matrices of 1024 x 1024 fp32) and 1.03 - 1.08 at r = 64:
 * there it loses a few percent of time and keeps the single rounding. */
int fa_set_lowrank_sum(fa_ctx* ctx, int part_id, const fa_lowrank_mat* mats, size_t M, int r_max);
/* The low-rank receipt of client `client_slot`: rank r <= r_max and f, len values, where len must be fa_lowrank_len(.., r)
 * (FA_ERR_ARG otherwise, as for r; the round stays as it was), under `weight` (rule 5).  flags: FA_HOST_PINNED as for
 * fa_submit_mx8.  Enqueues the H2D of f to every GPU that holds part of the part, into the slot's shadow (allocated at the
 * part's first submit); the slot then counts as submitted.  FA_ERR_STATE on a part without fa_set_lowrank_sum. */
int fa_submit_lowrank_sum(fa_ctx* ctx, int part_id, int client_slot, const float* f, size_t len, int r, float weight,
                          int flags);

/* Rot1 receipts (the header comment, "Rot1 receipts"): Hadamard sign codes, expanded on the GPU by fp16 MFMA. */
#define FA_ROT1_BLOCK 4096
/* The uint32 words of `bits` and the fp32 values of `scale` for a bucket of n elements: 128 and 1 per block. */
size_t fa_rot1_words(size_t n);
size_t fa_rot1_blocks(size_t n);
/* Encode rules 2-5 on the n given deltas of a whole bucket, pure host arithmetic, usable without a device: bits gets
 * fa_rot1_words(n) words, scale fa_rot1_blocks(n) values. */
int fa_rot1_encode(const float* delta, size_t n, uint64_t seed, uint32_t* bits, float* scale);
/* The decoder, pure host arithmetic: d[i] = the delta of bucket element idx0 + i over cnt elements.  bits and scale
 * start at block idx0 >> 12 and cover the range. */
int fa_rot1_decode(const uint32_t* bits, const float* scale, uint64_t seed, uint64_t idx0, size_t cnt, float* d);
/* The expansion on raw device pointers, on device `gpu`: d_dst[i] (cnt of dst_dtype) = fl(widen(d_ref[i]) + d_i), or d_i
 * with d_ref NULL (absolute mode), over bucket elements idx0 .. idx0 + cnt - 1 with any idx0.  d_bits and d_scale start
 * at block idx0 >> 12 and cover the range: a block that the range holds part of is transformed whole and stored only
 * inside the range, and every store is checked against the range.  ctx may be NULL (then `gpu` is the HIP device).
 * Every argument is checked before any device call: the dtypes and their pair ((dst, ref) as (in, out)), idx0 + cnt <
 * 2^64, and for cnt > 0 null pointers and alignment (FA_ERR_ALIGN: d_bits and d_scale 4 bytes, d_ref and d_dst their
 * element); with cnt == 0 and valid arguments it returns FA_OK without touching a device.  Any element phase of d_ref
 * and d_dst is correct; a lane moves its four consecutive elements in one access (16 bytes of fp32, 8 of a 16-bit type)
 * where every pointer is so aligned at the bucket's multiples of four.  d_dst must not overlap d_ref.  Async on
 * hip_stream (NULL = the ctx's compute stream of `gpu`, or the null stream). */
int fa_rot1_expand_device(fa_ctx* ctx, int gpu, const uint32_t* d_bits, const float* d_scale, uint64_t seed, uint64_t idx0,
                          size_t cnt, const void* d_ref, fa_dtype ref_dtype, void* d_dst, fa_dtype dst_dtype,
                          void* hip_stream);
/* Encode rules 1-6 on raw device pointers, on device `gpu`: over the n elements of d_new and d_sent (one dtype), bucket
 * elements idx0 .. idx0 + n - 1 with idx0 a multiple of 4096 (FA_ERR_ARG otherwise), d_bits gets fa_rot1_words(n) words
 * and d_scale fa_rot1_blocks(n) values (block idx0 >> 12 first) and, unless d_out is NULL, d_out gets g' (n elements of
 * the same dtype).  d_out may be d_sent or d_new exactly or overlap neither (FA_ERR_ARG otherwise).  One launch, a
 * workgroup per block.  The checks, ctx == NULL, the n == 0 probe and the stream are fa_rot1_expand_device's; 16-byte
 * accesses are used where d_new, d_sent and d_out are 16-byte aligned. */
int fa_rot1_encode_device(fa_ctx* ctx, int gpu, const void* d_new, fa_dtype new_dtype, const void* d_sent,
                          fa_dtype sent_dtype, size_t n, uint64_t idx0, uint64_t seed, uint32_t* d_bits, float* d_scale,
                          void* d_out, void* hip_stream);
/* Lets a part take rot1 receipts (part_id >= 0), or sets the context default for parts defined later (part_id < 0).  It
 * is the stage of fa_set_mx8 with a fourth format: admission, the reference, the refusals (FA_LITERAL,
 * FA_SHARD_CLIENT_RS, a secagg part) and the call ordering are fa_set_mx8's, the part is never kept host-side and
 * FA_ACCUMULATE_ON_ARRIVAL leaves it non-eager.  A part may take all four formats, and different owners may send
 * different ones.  Memory: per GPU and client slot a shadow of 516 bytes per block its range touches, rounded up to 256,
 * allocated at the part's first fa_submit_rot1; on == 0 frees it. */
int fa_set_rot1(fa_ctx* ctx, int part_id, int on);
/* A rot1 receipt of client `client_slot`: bits (fa_rot1_words(n) words), scale (fa_rot1_blocks(n) values) and the seed.
 * flags: FA_HOST_PINNED as for fa_submit_mx8 (bits and scale stay unchanged until fa_finalize* returns);
 * FA_ROT1_ABSOLUTE = absolute mode (x = d).  Per GPU enqueues the H2D of the words and scales of the blocks its element
 * range touches, then per piece the expansion with that range's idx0, ordered after the part's last reducing call and
 * before the next.  The slot then counts as the client's receipt exactly as after fa_submit.  The reference and its
 * FA_ERR_STATE are fa_submit_mx8's; FA_ERR_STATE on a part without fa_set_rot1. */
#define FA_ROT1_ABSOLUTE 0x2
int fa_submit_rot1(fa_ctx* ctx, int part_id, int client_slot, const uint32_t* bits, const float* scale, uint64_t seed,
                   float weight, int flags);

/* Rot1-sum stage (the header comment, "Rot1-sum stage"): rot1 receipts reduced in the rotated domain, without expanding
 * them. */
#define FA_ROT1_SUM_MAX_CLIENTS 128
/* Rules 0-6 on the host, usable without a device: out[i] (fp32, cnt elements) is the aggregate of bucket element idx0 + i
 * from the receipts (bits[c], scale[c], seed[c]) under w[c], c < D, and ref (fp32, cnt elements, NULL = absolute mode).
 * bits[c] and scale[c] start at block idx0 >> 12 and cover the range.  FA_ERR_ARG as fa_rot1_sum_device. */
int fa_rot1_sum_host(const uint32_t* const* bits, const float* const* scale, const uint64_t* seed, const float* w, int D,
                     uint64_t idx0, size_t cnt, const float* ref, float* out);
/* Rules 0-6 on raw device pointers, on device `gpu`, over bucket elements idx0 .. idx0 + cnt - 1 with any idx0: d_out[i]
 * (cnt of out_dtype, one rounding) from d_ref (cnt of ref_dtype, NULL = absolute mode) and the receipts: d_bits[c] and
 * d_scale[c] are device memory, start at block idx0 >> 12 and cover the range (128 words and one scale per block); a
 * block that the range holds part of is reduced whole and stored only inside the range, every store checked against
 * it.  The arrays d_bits, d_scale, seed and w themselves are host memory and are read before the call returns.  ctx may
 * be NULL (then `gpu` is the HIP device).  Every argument is checked before any device call: the dtypes and their pair
 * (bf16 <-> f16: FA_ERR_ARG), 1 <= D <= FA_ROT1_SUM_MAX_CLIENTS, idx0 + cnt < 2^64, and for cnt > 0 null pointers, alignment
 * (FA_ERR_ALIGN: every d_bits[c] and d_scale[c] 4 bytes, d_ref and d_out their element) and that d_out does not overlap
 * d_ref (FA_ERR_ARG); with cnt == 0 and valid arguments it returns FA_OK without touching a device.  Any element phase of
 * d_ref and d_out is correct; a lane moves its 16 consecutive elements in 16-byte accesses where both are 16-byte aligned
 * at the bucket's multiples of 16, and the bits do not depend on it.  One launch, a workgroup per block.  Async on
 * hip_stream (NULL = the ctx's compute stream of `gpu`, or the null stream). */
int fa_rot1_sum_device(fa_ctx* ctx, int gpu, const uint32_t* const* d_bits, const float* const* d_scale, const uint64_t* seed,
                       const float* w, int D, uint64_t idx0, size_t cnt, const void* d_ref, fa_dtype ref_dtype, void* d_out,
                       fa_dtype out_dtype, void* hip_stream);
/* Gives a part the stage (part_id >= 0, on != 0): its rounds take rot1 receipts with fa_submit_rot1_sum and reduce them by
 * rules 0-6 against the part's last output; the round under way is dropped.  Again on a part that has it: nothing.  on == 0
 * removes the stage and frees what it allocated.  FA_ERR_ARG, naming the cause: D > FA_ROT1_SUM_MAX_CLIENTS, part_id < 0 (no
 * context default), a part whose mode is not FA_FEDAVG, a part with a clip, Krum, DnC, geomed, secagg, sign, sparse-sum,
 * MX8-sum, low-rank-sum or receipt stage (those setters refuse a rot1-sum part in turn), an FA_SHARD_CLIENT_RS context.
 * In DESIGN.md 8s the stage takes 0.132 / 0.058 / 0.048 of the expanded route's device time with one seed and 0.42 / 0.41 /
 * 0.41 with a seed per owner (D = 8 / 32 / 64, n = 64 Mi fp32): it lost nowhere, but a seed per owner costs one transform
 * per owner and block, about 8 times a round with one seed at D = 64. */
int fa_set_rot1_sum(fa_ctx* ctx, int part_id, int on);
/* The rot1 receipt of client `client_slot`: bits (fa_rot1_words(n) words), scale (fa_rot1_blocks(n) values) and the seed
 * of the whole bucket, under `weight` (rule 7).  flags: FA_HOST_PINNED as for fa_submit_rot1.  Per GPU enqueues the H2D of
 * the words and scales of the blocks its range touches into the slot's shadow (the rot1 shadow layout, allocated at the
 * part's first submit); the slot then counts as submitted.  FA_ERR_STATE on a part without fa_set_rot1_sum. */
int fa_submit_rot1_sum(fa_ctx* ctx, int part_id, int client_slot, const uint32_t* bits, const float* scale, uint64_t seed,
                       float weight, int flags);

/* Secagg stage (the header comment, "Secagg stage"): masked uint32 sums unmasked and decoded on the GPU. */
#define FA_SECAGG_MAX_TERMS 4096
/* Gives a part the stage with the decoding scale (part_id >= 0; again: only the scale changes); scale <= 0 removes it
 * with its term table.  FA_ERR_ARG, naming the cause: scale NaN or +inf, part_id < 0 (no context default), a part
 * whose mode is not FA_FEDAVG or whose `in` is not FA_F32, a part of more than 2^36 elements, a part with a clip,
 * Krum, geomed or MX8 stage (those setters refuse a secagg part in turn), an FA_SHARD_CLIENT_RS context. */
int fa_set_secagg(fa_ctx* ctx, int part_id, float scale);
/* The terms of the part's next reducing call: keys (8 T words), nonces (3 T words), signs (T ints, each +1 or -1), all
 * host arrays, copied before the return; NULL allowed with T == 0.  FA_ERR_ARG: T outside 0 .. FA_SECAGG_MAX_TERMS, a
 * null array, another sign.  FA_ERR_STATE on a part without the stage.  A reducing call uses the terms and drops
 * them. */
int fa_secagg_set_terms(fa_ctx* ctx, int part_id, int T, const uint32_t* keys, const uint32_t* nonces, const int* signs);
/* Rules 2-4 on raw device pointers: d_out[i] (n of `out`, one rounding) = the decoded sum of the D buckets d_clients
 * (n uint32 words each, bucket elements idx0 .. idx0 + n - 1) and the T terms, on device `gpu`.  ctx may be NULL (then
 * `gpu` is the HIP device; D > 128 with a 16-bit output needs one, for scratch).  Every argument is checked before any
 * device call: D >= 1, the out dtype, scale (finite, > 0), the terms as above, idx0 + n <= 2^36, and for n > 0 null
 * pointers and element alignment (FA_ERR_ALIGN); with n == 0 and valid arguments it returns FA_OK without touching a
 * device.  Otherwise it uploads the terms, enqueues on hip_stream (NULL = the ctx's compute stream of `gpu`, or the
 * null stream) and waits for it.  Any element phase of the pointers is correct; 16-byte loads are used where every
 * pointer is 16-byte aligned at the first multiple of 16 of the bucket index. */
int fa_secagg_unmask_device(fa_ctx* ctx, int gpu, const void* const* d_clients, int D, size_t n, uint64_t idx0, int T,
                            const uint32_t* keys, const uint32_t* nonces, const int* signs, float scale, void* d_out,
                            fa_dtype out, void* hip_stream);
/* Rule 2, pure host arithmetic, usable without a device: out[0, n) = the mask words of bucket elements idx0 .. idx0 +
 * n - 1 under key (8 words) and nonce (3 words) -- the owner's side, and the bits the kernel removes. */
int fa_secagg_mask_host(const uint32_t* key, const uint32_t* nonce, uint64_t idx0, size_t n, uint32_t* out);
/* The owner's fixed-point codes, pure host arithmetic: out[i] = rint((double)v[i] * (double)q), ties to even,
 * saturated at +-(2^31 - 1); a NaN gives 0 and is counted in *n_bad (nullable).  q finite and > 0; the server decodes
 * with scale = 1 / q. */
int fa_secagg_quantize(const float* v, size_t n, float q, int32_t* out, uint64_t* n_bad);
/* Which vector form a launch over n elements and T terms takes: 0 = a tile per wave, 1 = the term split (the four
 * waves of a workgroup share a tile's terms).  Pure host arithmetic; the bits do not depend on it. */
int fa_secagg_form(size_t n, int T);

/* Sign-vote stage (the header comment, "Sign-vote stage"): one-bit receipts counted bit-sliced on the GPU. */
#define FA_SIGN_MAX_CLIENTS 128
#define FA_SIGN_MAJORITY 0
#define FA_SIGN_MEAN 1
/* ceil(n / 32): the words of a sign receipt, and of a vote plane, of n elements. */
size_t fa_sign_words(size_t n);
/* Rule 2, pure host arithmetic: bits (fa_sign_words(n) words) = the sign receipt of the n deltas. */
int fa_sign_pack(const float* delta, size_t n, uint32_t* bits);
/* Rules 3-9 on the host, usable without a device: bits[k], k < D, are whole receipts; element i of ref (fp32, n
 * elements, NULL = absolute mode), out (the fp32 a_i, before any rounding to a 16-bit type), neg and pos (fa_sign_words(n)
 * words each, both NULL or both set, majority only) is bucket element idx0 + i, idx0 a multiple of 32.  FA_ERR_ARG as
 * fa_sign_vote_device. */
int fa_sign_vote_host(const uint32_t* const* bits, int D, size_t n, uint64_t idx0, float eta, int rule, int margin,
                      const float* ref, float* out, uint32_t* neg, uint32_t* pos);
/* Rules 3-9 on raw device pointers: d_out[i] (n of out_dtype, one rounding) from the D receipts d_bits (each the whole
 * receipt of its bucket: the call reads its words idx0 >> 5 .. ) and d_ref (n of ref_dtype, NULL = absolute mode), element
 * i being bucket element idx0 + i; d_neg and d_pos (fa_sign_words(n) words each, both NULL or both set, majority only) get
 * the planes.  ctx may be NULL (then `gpu` is the HIP device).  Every argument is checked before any device call: 1 <= D
 * <= FA_SIGN_MAX_CLIENTS, the dtypes and their pair (bf16 <-> f16: FA_ERR_ARG), eta finite and > 0, the rule, 1 <= margin
 * <= D, idx0 a multiple of 32 with idx0 + n < 2^64, one plane pointer without the other, planes under the mean rule, and
 * for n > 0 null pointers, alignment (FA_ERR_ALIGN: receipts and planes 4 bytes, d_ref and d_out their element) and that
 * d_out does not overlap d_ref; with n == 0 and valid arguments it returns FA_OK without touching a device.  Async on
 * hip_stream (NULL = the ctx's compute stream of `gpu`, or the null stream).  Any phase of the pointers is correct; the
 * vector form needs the receipts (at word idx0 >> 5) and the planes in one 16-byte phase and d_ref, d_out 16-byte
 * aligned (fa_sign_form). */
int fa_sign_vote_device(fa_ctx* ctx, int gpu, const uint32_t* const* d_bits, int D, size_t n, uint64_t idx0, float eta,
                        int rule, int margin, const void* d_ref, fa_dtype ref_dtype, void* d_out, fa_dtype out_dtype,
                        uint32_t* d_neg, uint32_t* d_pos, void* hip_stream);
/* Which form fa_sign_vote_device takes for these operands: 0 = the element form throughout, 1 = the vector form with
 * element edges.  Pure host arithmetic on the pointer values; the bits do not depend on it. */
int fa_sign_form(size_t n, const uint32_t* const* d_bits, int D, uint64_t idx0, const void* d_ref, fa_dtype ref_dtype,
                 const void* d_out, fa_dtype out_dtype, const void* d_neg, const void* d_pos);
/* Gives a part the stage (part_id >= 0; again: the numbers change, a round under way stays); eta <= 0 removes it and
 * frees what it allocated.  planes != 0: the reducing calls leave the vote planes (rule 9).  FA_ERR_ARG, naming the
 * cause: eta NaN or +inf, a rule other than the two, margin outside 1 .. D, D > FA_SIGN_MAX_CLIENTS, part_id < 0 (no
 * context default), a part whose mode is not FA_FEDAVG, a part with a clip, Krum, DnC, geomed, secagg or receipt stage
 * (those setters refuse a sign part in turn), an FA_SHARD_CLIENT_RS context.  FA_ERR_STATE: planes under the mean rule
 * or on a part with a noise stage or a server optimizer. */
int fa_set_sign(fa_ctx* ctx, int part_id, float eta, int rule, int margin, int planes);
/* The sign receipt of client `client_slot`: bits (fa_sign_words(n) words).  flags: FA_HOST_PINNED as for fa_submit_rot1.
 * Per GPU enqueues the H2D of the words of its range into the slot's shadow (allocated at the part's first submit); the
 * slot then counts as submitted.  FA_ERR_STATE on a part without fa_set_sign. */
int fa_submit_sign(fa_ctx* ctx, int part_id, int client_slot, const uint32_t* bits, int flags);
/* The planes of the part's last reducing call into host arrays of fa_sign_words(n) words each, waiting for it.
 * FA_ERR_STATE on a part without planes or not yet reduced with them. */
int fa_copy_sign_planes(fa_ctx* ctx, int part_id, uint32_t* neg, uint32_t* pos);

/* Sparse-sum stage (the header comment, "Sparse-sum stage"): top-k receipts reduced on the GPU without expanding them. */
#define FA_SPARSE_MAX_CLIENTS 128
/* fa_sparse_sum_form: a bit each. */
#define FA_SPARSE_VECTOR 1   /* the dense side moves 16 bytes per access wherever a lane lies inside the launch */
#define FA_SPARSE_BIG_TILE 2 /* a wave owns 8192 elements, not 2048: densities below 1 / 2048 */
/* Rules 1-2 on the host, usable without a device: out[i] (fp32, n elements) is the aggregate of bucket element idx0 + i
 * from the receipts (idx[c], val[c]) of k[c] entries under w[c], c < D, and ref (fp32, n elements, NULL = absolute mode).
 * Entries outside [idx0, idx0 + n) are skipped.  FA_ERR_ARG as fa_sparse_sum_device. */
int fa_sparse_sum_host(const uint32_t* const* idx, const float* const* val, const size_t* k, const float* w, int D, size_t n,
                       uint64_t idx0, const float* ref, float* out);
/* The bytes of d_work for one fa_sparse_sum_device over n elements and D clients. */
size_t fa_sparse_sum_workspace(size_t n, int D);
/* Rules 1-2 on raw device pointers over bucket elements idx0 .. idx0 + n - 1: d_out[i] (n of out_dtype, one rounding)
 * from d_ref (n of ref_dtype, NULL = absolute mode) and the receipts: d_idx[c] and d_val[c] are client c's k[c] entries,
 * the whole bucket's or a range's (entries outside the range are skipped); the arrays d_idx, d_val, k and w themselves
 * are host memory and are read before the call returns.  d_work: fa_sparse_sum_workspace(n, D) bytes, 16-byte aligned,
 * not initialised, the call's own until it has run.  ctx may be NULL (then `gpu` is the HIP device).  Every argument is
 * checked before any device call: 1 <= D <= FA_SPARSE_MAX_CLIENTS, the dtypes and their pair (bf16 <-> f16: FA_ERR_ARG),
 * idx0 + n < 2^64 (and <= 2^32 where a receipt has entries), k[c] <= 2^32 - 1, and for n > 0 null pointers, alignment
 * (FA_ERR_ALIGN: idx and val 4 bytes, d_ref and d_out their element, d_work 16) and that d_out does not overlap d_ref;
 * with n == 0 and valid arguments it returns FA_OK without touching a device.  Ascending order is the caller's
 * obligation, as in fa_topk_expand_device: with unsorted or repeated indices the values are unspecified, nothing is
 * written outside d_out[0, n) and nothing is read outside idx[0, k) and val[0, k).  Async on hip_stream (NULL = the ctx's
 * compute stream of `gpu`, or the null stream).  Any phase of the pointers is correct (fa_sparse_sum_form). */
int fa_sparse_sum_device(fa_ctx* ctx, int gpu, const uint32_t* const* d_idx, const float* const* d_val, const size_t* k,
                         const float* w, int D, size_t n, uint64_t idx0, const void* d_ref, fa_dtype ref_dtype, void* d_out,
                         fa_dtype out_dtype, void* d_work, void* hip_stream);
/* Which form fa_sparse_sum_device takes for these operands: FA_SPARSE_VECTOR if d_ref and d_out agree on a common head
 * before their 16-byte boundaries (else the dense side goes element by element), FA_SPARSE_BIG_TILE by the density
 * sum k / (D n).  Pure host arithmetic on the counts and the pointer values; the bits do not depend on it. */
int fa_sparse_sum_form(size_t n, const size_t* k, int D, const void* d_ref, fa_dtype ref_dtype, const void* d_out,
                       fa_dtype out_dtype);
/* Gives a part the stage (part_id >= 0): its rounds take top-k receipts of at most k_max entries (fa_submit_sparse) and
 * reduce them by rules 1-2 against the part's last output; again: k_max changes, the shadows are allocated anew, the round
 * under way is dropped if they were in use, and the reference stays (rule 4).  k_max == 0 removes the stage and frees what it allocated.  FA_ERR_ARG, naming
 * the cause: D > FA_SPARSE_MAX_CLIENTS, part_id < 0 (no context default), a part whose mode is not FA_FEDAVG, a part with
 * a clip, Krum, DnC, geomed, secagg, sign or receipt stage (those setters refuse a sparse-sum part in turn), an
 * FA_SHARD_CLIENT_RS context.  No density limit is enforced: in DESIGN.md 8p the stage beats the expanded route at every
 * density measured, k = n / 1000 to n / 10; nothing above n / 10 was measured. */
int fa_set_sparse_sum(fa_ctx* ctx, int part_id, size_t k_max);
/* The top-k receipt of client `client_slot`: k <= k_max entries, idx strictly ascending and < n (checked on the host:
 * FA_ERR_ARG naming the entry, the round stays as it was), under `weight` (rule 3).  flags: FA_HOST_PINNED as for
 * fa_submit_topk.  Per GPU enqueues the H2D of the entries of its range into the slot's shadow (allocated at the part's
 * first submit); the slot then counts as submitted.  FA_ERR_STATE on a part without fa_set_sparse_sum. */
int fa_submit_sparse(fa_ctx* ctx, int part_id, int client_slot, const uint32_t* idx, const float* val, size_t k, float weight,
                     int flags);

/* MX8-sum stage (the header comment, "MX8-sum stage"): MX8 receipts reduced on the GPU without expanding them. */
#define FA_MX8_SUM_MAX_CLIENTS 128
/* fa_mx8_sum_form. */
#define FA_MX8_SUM_VECTOR 1 /* 16 elements per lane: 16-byte accesses to q, the reference and the output */
/* Rules 1-3 on the host, usable without a device: out[i] (fp32, n elements) is the aggregate of bucket element idx0 + i
 * from the receipts (q[c], e[c]) under w[c], c < D, and ref (fp32, n elements, NULL = absolute mode).  q[c][i] is the code
 * of bucket element idx0 + i, e[c][0] the scale of the block that element idx0 lies in.  FA_ERR_ARG as fa_mx8_sum_device. */
int fa_mx8_sum_host(const int8_t* const* q, const uint8_t* const* e, const float* w, int D, size_t n, uint64_t idx0,
                    const float* ref, float* out);
/* Rules 1-3 on raw device pointers over bucket elements idx0 .. idx0 + n - 1: d_out[i] (n of out_dtype, one rounding) from
 * d_ref (n of ref_dtype, NULL = absolute mode) and the receipts: d_q[c] are client c's n codes, d_e[c] the scale bytes of
 * blocks idx0 >> 5 .. (idx0 + n - 1) >> 5; the arrays d_q, d_e and w themselves are host memory and are read before the
 * call returns.  ctx may be NULL (then `gpu` is the HIP device).  Every argument is checked before any device call: 1 <= D
 * <= FA_MX8_SUM_MAX_CLIENTS, the dtypes and their pair (bf16 <-> f16: FA_ERR_ARG), idx0 + n < 2^64, and for n > 0 null
 * pointers, the element alignment of d_ref and d_out (FA_ERR_ALIGN) and that d_out does not overlap d_ref; with n == 0
 * and valid arguments it returns FA_OK without touching a device.  Nothing is read outside q[0, n) and those scale bytes,
 * nothing is written outside d_out[0, n).  Async on hip_stream (NULL = the ctx's compute stream of `gpu`, or the null
 * stream).  Any phase of the pointers and any idx0 is correct (fa_mx8_sum_form). */
int fa_mx8_sum_device(fa_ctx* ctx, int gpu, const int8_t* const* d_q, const uint8_t* const* d_e, const float* w, int D, size_t n,
                      uint64_t idx0, const void* d_ref, fa_dtype ref_dtype, void* d_out, fa_dtype out_dtype, void* hip_stream);
/* Which form fa_mx8_sum_device takes for these operands: FA_MX8_SUM_VECTOR if d_ref and d_out agree on a common head before
 * their 16-byte boundaries, every d_q[c] is 16-byte aligned after that head and the bucket index of the first element
 * after it is a multiple of 16; else 0, the element form.  (A launch that ends before the head has no vector in either
 * case.)  Pure host arithmetic on the pointer values; the bits do not depend on it. */
int fa_mx8_sum_form(size_t n, const int8_t* const* d_q, int D, uint64_t idx0, const void* d_ref, fa_dtype ref_dtype,
                    const void* d_out, fa_dtype out_dtype);
/* Gives a part the stage (part_id >= 0, on != 0): its rounds take MX8 receipts with fa_submit_mx8_sum and reduce them by
 * rules 1-3 against the part's last output; the round under way is dropped.  Again on a part that has it: nothing.  on == 0
 * removes the stage and frees what it allocated.  FA_ERR_ARG, naming the cause: D > FA_MX8_SUM_MAX_CLIENTS, part_id < 0 (no
 * context default), a part whose mode is not FA_FEDAVG, a part with a clip, Krum, DnC, geomed, secagg, sign, sparse-sum or
 * receipt stage (those setters refuse an MX8-sum part in turn), an FA_SHARD_CLIENT_RS context.  In DESIGN.md 8q the stage takes
 * 0.105 - 0.176 of the expanded route's device time at every D measured (64, 32, 8; n = 64 Mi fp32); it lost nowhere. */
int fa_set_mx8_sum(fa_ctx* ctx, int part_id, int on);
/* The MX8 receipt of client `client_slot`, q (n int8) and e (ceil(n / 32) bytes) of the whole bucket, under `weight` (rule
 * 4).  flags: FA_HOST_PINNED as for fa_submit_mx8.  Per GPU enqueues the H2D of its range's q bytes and scale bytes into
 * the slot's shadow (allocated at the part's first submit); the slot then counts as submitted.  FA_ERR_STATE on a part
 * without fa_set_mx8_sum. */
int fa_submit_mx8_sum(fa_ctx* ctx, int part_id, int client_slot, const int8_t* q, const uint8_t* e, float weight, int flags);

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
