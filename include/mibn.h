/*
 * mibn - MI355X-native exact inference backend for sorobn-style Bayesian networks.
 *
 * C-ABI drop-in boundary for the hot path of MaxHalford/sorobn:
 *
 *   BayesNet.query(..., algorithm="exact")   sorobn/bayes_net.py:796-875
 *     -> BayesNet._variable_elimination      sorobn/bayes_net.py:739-794
 *          -> pointwise_mul / pointwise_mul_two   sorobn/bayes_net.py:233-256
 *          -> CDTAccessor.sum_out                 sorobn/bayes_net.py:100-103
 *   BayesNet.query(..., algorithm="gibbs")   sorobn/bayes_net.py:665-737
 *
 * The reference is pure Python with no FFI; the seam is the method boundary
 * `_variable_elimination(*query, event=...) -> pd.Series` (bayes_net.py:739, called from 848) and
 * `_gibbs_sampling(*query, event=..., n_iterations=...)` (bayes_net.py:665, called from 851-853).
 * A Python caller flattens the pandas CPTs once (mibn_set_network) and then answers batches of
 * requests through mibn_query_batch; labels <-> codes and pandas objects stay on the Python side
 * (sorobn_amd/bayes_net.py; binding shown in INTEGRATION.md).
 *
 * Conventions: plain C types only; every function returns 0 on success or a negative MIBN_E_*
 * code, with a message available from mibn_last_error(); the caller owns all host buffers, the
 * library owns all device memory; one host thread per handle (thread-compatible, not thread-safe).
 * There is NO CPU fallback: mibn_create fails with MIBN_E_NODEVICE when no gfx950 device is
 * visible.
 */
#ifndef MIBN_H
#define MIBN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIBN_OK 0
#define MIBN_E_ARG (-1)       /* invalid argument */
#define MIBN_E_NODEVICE (-2)  /* no HIP device / wrong architecture */
#define MIBN_E_HIP (-3)       /* HIP runtime error */
#define MIBN_E_NOMEM (-4)     /* plan needs more device memory than the arena budget */
#define MIBN_E_STATE (-5)     /* call order (e.g. query before set_network) */
#define MIBN_E_LIMIT (-6)     /* a compile-time limit (scope size, axes) was exceeded */
#define MIBN_E_COMM (-7)      /* RCCL missing or a collective failed */

typedef struct mibn_ctx mibn_t;

/* Number of visible HIP devices (0 when there is no GPU/driver). Never fails hard. */
int mibn_device_count(int *count);

/* Library version string (static storage). */
const char *mibn_version(void);

/* Create a context bound to HIP device `device`. */
int mibn_create(int device, mibn_t **out);
void mibn_destroy(mibn_t *h);
const char *mibn_last_error(const mibn_t *h);

/*
 * Install the network (replaces `self.P` of the reference, bayes_net.py:324, after prepare()).
 *   n_vars             variables 0..n_vars-1; variable v owns exactly one CPT, factor v
 *   card[n_vars]       cardinality of each variable (size of its sorted label domain)
 *   scope_off[n_vars+1], scope_vars[]   CSR: scope of factor v = scope_vars[scope_off[v]..]
 *                      = [*parents(v), v] - the level order of the reference's CPT Series
 *   value_off[n_vars+1], values[]       dense float64 table of factor v in C-order over its scope
 *                      (last scope entry fastest), absent rows = 0.0
 */
int mibn_set_network(mibn_t *h, int32_t n_vars, const int32_t *card, const int64_t *scope_off,
                     const int32_t *scope_vars, const int64_t *value_off, const double *values);

/*
 * Optional elimination-order hints: n_hints priority arrays of n_vars entries (lower = earlier).
 * The planner evaluates every hint next to its built-in candidate orders with the section 8(d)
 * cost model and executes the cheapest.  Orders change only floating-point rounding (~1e-16), not
 * the answer (the reference's own order is an arbitrary set-iteration order, bayes_net.py:766,779).
 */
int mibn_set_order_hints(mibn_t *h, int32_t n_hints, const int32_t *priorities);

/*
 * Answer a batch of exact posterior queries (= B calls of BayesNet._variable_elimination followed
 * by the normalisation of bayes_net.py:790).
 *   q_off[B+1], q_vars[]   CSR: query variables of request b, in the caller's argument order
 *   e_off[B+1], e_vars[], e_codes[]   CSR: evidence variables and their label codes; a code of -1
 *                          (label outside the domain) yields an all-zero posterior, like the
 *                          reference's empty Series
 *   out_off[B+1], out[]    dense posterior of request b at out[out_off[b]..out_off[b+1]) in C-order
 *                          over its query variables (last query variable fastest); all zeros when
 *                          the evidence has probability 0
 * Errors: MIBN_E_ARG for unknown variables, duplicates or query/evidence overlap.
 */
int mibn_query_batch(mibn_t *h, int64_t B, const int64_t *q_off, const int32_t *q_vars,
                     const int64_t *e_off, const int32_t *e_vars, const int32_t *e_codes,
                     const int64_t *out_off, double *out);

/*
 * mibn_query_batch with per-call flags (nothing engine-wide changes, so it is safe next to asynchronous calls in flight
 * on other engines of the same network):
 *   MIBN_Q_NOPRUNE   multiply every CPT instead of pruning to the ancestors of the query / evidence variables
 *                    (bayes_net.py:763-765): the semantics of full_joint_dist / predict_proba (bayes_net.py:460), where
 *                    with sparse or unnormalised CPTs a barren node does not sum to 1.
 *   MIBN_Q_UNNORMALISED  write sum_hidden prod factors = P(q, e), the joint, instead of the posterior P(q | e) (same C-order, no
 *                    division by the sum).  A request may then have ZERO query variables: its out slice is one cell, P(e) - the
 *                    probability of the evidence.  Zero-probability evidence or a code of -1 gives 0; empty evidence gives 1.0
 *                    with pruning (the relevant set is empty) and Z = the mass of the product of every CPT with MIBN_Q_NOPRUNE.
 *                    May be combined with MIBN_Q_NOPRUNE.  Without it, zero query variables are rejected as before.  Flagged
 *                    calls are planned by the host's workers (no device planner, no plan templates, no adaptive policy: the
 *                    options gpu_emit / gpu_search do not change their results, and the call writes no option or policy state).
 */
#define MIBN_Q_NOPRUNE 1
#define MIBN_Q_UNNORMALISED 2
int mibn_query_batch_ex(mibn_t *h, uint32_t flags, int64_t B, const int64_t *q_off, const int32_t *q_vars,
                        const int64_t *e_off, const int32_t *e_vars, const int32_t *e_codes,
                        const int64_t *out_off, double *out);

/*
 * Most probable explanation: for each request b, codes[b*n_vars + v] = the label code of v in argmax_x P(x, e_b) over every
 * variable not in e_b (evidence variables carry their code), log_p[b] = natural log of that joint probability.
 *   e_off[B+1], e_vars[], e_codes[]   CSR evidence, as in mibn_query_batch (no query variables: every other variable is maximised)
 *   codes[B*n_vars], log_p[B]         outputs
 * Max-product variable elimination (every CPT, no pruning), one elimination step per variable, each writing an argmax table that a
 * traceback kernel decodes on the device.  Ties go to the lowest code.  Zero-probability evidence (or a code of -1) gives
 * log_p = -inf and code -1 for every non-evidence variable; single-state non-evidence variables get code 0.  Blocking and
 * host-planned, chunked by the arena budget; it changes no option and no state a later query call reads.  mibn_last_stats /
 * mibn_last_kernel_stats ("ve_max_kernel", "mpe_traceback_kernel") describe it; alg_bytes includes the argmax bytes written.
 * Errors: MIBN_E_ARG for unknown or duplicate evidence variables; MIBN_E_LIMIT for a variable of more than 65 536 states.
 */
int mibn_mpe_batch(mibn_t *h, int64_t B, const int64_t *e_off, const int32_t *e_vars, const int32_t *e_codes,
                   int32_t *codes, double *log_p);

/*
 * Expected counts (the E-step of BayesNet.fit_em): the requests run exactly as mibn_query_batch_ex(flags | MIBN_Q_UNNORMALISED) runs
 * them (blocking, host-planned; MIBN_Q_NOPRUNE may be or-ed in), but the slices P(q_b, e_b) stay on the device, where expect_kernel
 * (csrc/expect_kernel.hip.h) adds every request's posterior into one accumulation buffer.  With s_b = the sum of slice b = P(e_b):
 *     acc[acc_base[b] + sum_k idx_k * acc_stride[q_off[b] + k]] += weight[b] * slice_b[idx] / s_b      (nothing when s_b == 0)
 *     p_out[b] = s_b
 *   acc_base[B], acc_stride[q_off[B]]   the target of request b: a base cell and one stride (cells, may be negative) per query
 *                          variable, in q_vars order; the strides of a request must address distinct cells
 *   weight[B] or NULL      per-request weight (NULL: 1.0)
 *   n_acc, acc             the accumulation buffer (host, in/out): the call ADDS to what the caller passes, so sub-batches chain
 *   p_out[B] or NULL       P(e_b) of every request; a request may have zero query variables (it only fills p_out)
 * Bitwise repeatable: the same call gives the same acc bits on every run, whatever the scheduling and the "threads" option - no
 * floating-point atomics; consecutive requests form slabs that one wave walks in order, slab partials are added in slab order.  The
 * order across calls is the caller's.  Fast when the requests are laid out target-table major (a slab's targets span at most 2048
 * cells; a request whose own targets span more takes a slower global path with the same ordering rule).
 * Errors: the query path's; MIBN_E_ARG for a target that leaves [0, n_acc) - checked on the host from base, strides and
 * cardinalities before anything is launched; MIBN_E_LIMIT for more than 8 query variables in a request.  mibn_last_stats /
 * mibn_last_kernel_stats ("expect_kernel": its three launches together) describe the call; like mibn_mpe_batch it changes no option
 * and no state a later query call reads.
 */
int mibn_expect_batch(mibn_t *h, uint32_t flags, int64_t B, const int64_t *q_off, const int32_t *q_vars,
                      const int64_t *e_off, const int32_t *e_vars, const int32_t *e_codes,
                      const int64_t *acc_base /*[B]*/, const int64_t *acc_stride /*[q_off[B]]*/,
                      const double *weight /*[B] or NULL*/,
                      int64_t n_acc, double *acc /*in/out, host*/, double *p_out /*[B] or NULL*/);

/*
 * Exact posterior sampling: independent samples of P(x | e_b) under the normalised joint, by forward filtering (one sum
 * elimination pass per request, every table kept) and backward sampling (one walk over the kept tables per sample).
 *   e_off[B+1], e_vars[], e_codes[]   CSR evidence, as in mibn_mpe_batch
 *   s_off[B+1]                        request b gets s_off[b+1] - s_off[b] samples; g = s_off[b] + i is the GLOBAL ROW INDEX of its
 *                                     i-th sample.  s_off[0] is usually 0; a caller that draws a later part of a stream (a shard, a
 *                                     request run alone) passes the index of its first row there
 *   codes[(s_off[B] - s_off[0]) * n_vars]   row g - s_off[0]: the label codes of sample g (evidence variables carry their code,
 *                                     single-state variables 0)
 *   p_e[B] or NULL                    the unnormalised mass of the evidence (the FINAL cell; P(e_b) where the CPTs are distributions)
 *   flags                             MIBN_DRAW_PRUNE: every CPT is a complete distribution (the caller's promise) - only evidence
 *                                     variables and their ancestors are eliminated and drawn backward, every other variable is
 *                                     drawn forward from its CPT row, in id order, in the same kernel.  Without it every CPT takes
 *                                     part (the rule of mibn_mpe_batch): the path of sparse or unnormalised CPTs
 * Random stream: Philox4x32-10 keyed by `seed`, counter (g, variable id) - the convention of mibn_sample.  The codes are a function
 * of (network, evidence, s_off, seed, flags) alone: bit for bit the same for any chunk, threads, arena budget or wave cut.
 * A draw of x: weights w_x = prod_j phi_j in input order, total = their sum in code order, u * total against the running sum, the
 * first x with u < acc, else the last x of positive weight - a zero-weight state is never returned.
 * Zero mass (or a code of -1): p_e = 0 and code -1 for every non-evidence variable, as in mibn_mpe_batch.  Blocking and
 * host-planned, chunked and cut into waves by the arena budget; it changes no option and no state a later query call reads, and
 * books nothing into the totals.  mibn_last_stats / mibn_last_kernel_stats ("ve_sum_kernel", "posterior_draw_kernel") describe it.
 * Errors: MIBN_E_ARG for unknown or duplicate evidence variables, a descending s_off or an unknown flag; MIBN_E_LIMIT for a
 * variable of more than 65 536 states or a network whose sample state (256 samples x n_vars codes) does not fit the LDS.
 */
#define MIBN_DRAW_PRUNE 1u
int mibn_posterior_sample_batch(mibn_t *h, int64_t B, const int64_t *e_off, const int32_t *e_vars, const int32_t *e_codes,
                                const int64_t *s_off, uint64_t seed, uint32_t flags, int32_t *codes, double *p_e);

/*
 * Marginal MAP: for each request b, the most probable joint assignment of its MAP variables M_b with every other non-evidence
 * variable summed out,  m*_b = argmax_m sum_h P(m, h, e_b):
 *   m_off[B+1], m_vars[]              CSR list of the MAP variables of every request (may be empty: no codes, log_p = log P(e_b))
 *   e_off[B+1], e_vars[], e_codes[]   CSR evidence, as in mibn_mpe_batch
 *   codes[m_off[B] - m_off[0]]        codes[m_off[b] - m_off[0] + k] = the label code of m_vars[m_off[b] + k] in m*_b
 *   log_p[B]                          natural log of max_m sum_h P(m, h, e_b) (unnormalised CPTs: of that mass)
 *   flags                             MIBN_MAP_PRUNE: every CPT is a complete distribution (the caller's promise) - only M_b, the
 *                                     evidence and their ancestors take part, a barren summed variable sums to 1.  Without it every
 *                                     CPT takes part (the rule of mibn_mpe_batch): the path of sparse or unnormalised CPTs
 * A two-phase elimination in one schedule (csrc/planner.h, "MAP programs"): the hidden variables are summed out first, then M_b is
 * maximised out - one step per variable, every max step with an argmax table that a traceback kernel decodes on the device.  The
 * dense joint over M_b is never built, but a step of the max phase holds the MAP variables that interact through the summed ones:
 * a request whose step would reach 2^31 cells is MIBN_E_LIMIT - inherent to marginal MAP (the maxima cannot move inside the sums).
 * Ties go to the lowest code; a single-state MAP variable gets code 0.  Zero mass (or a code of -1): log_p = -inf and code -1 for
 * every MAP variable.  A request with an empty program (M empty, no evidence, MIBN_MAP_PRUNE) has log_p = 0.
 * The result is a function of (network, request, flags) alone: bit for bit the same for any chunk, threads or arena budget.
 * Blocking and host-planned, chunked and cut into waves by the arena budget; it changes no option and no state a later query call
 * reads, and books nothing into the totals.  mibn_last_stats / mibn_last_kernel_stats ("ve_map_kernel", "map_traceback_kernel")
 * describe it; the rows "ve_map_kernel:sum tiles" / "ve_map_kernel:max tiles" are no kernels but what the level launches held
 * beside segments: launches = sum / max steps that ran as GENERIC tiles, items = their workgroups (no time and no bytes of their
 * own: both are booked under "ve_map_kernel", so the rows' alg_bytes add up without counting anything twice).
 * Errors: MIBN_E_ARG for unknown or duplicate variables, a variable both in M_b and in the evidence, a descending m_off or an
 * unknown flag; MIBN_E_LIMIT for a MAP variable of more than 65 536 states (argmax entries are 16 bits) and for the planner's cell
 * limit; MIBN_E_NOMEM as in the other elimination calls.  The 65 536-state limit is checked before the requests are validated: a
 * call that breaks both returns MIBN_E_LIMIT.
 */
#define MIBN_MAP_PRUNE 1u
int mibn_map_batch(mibn_t *h, uint32_t flags, int64_t B, const int64_t *m_off, const int32_t *m_vars,
                   const int64_t *e_off, const int32_t *e_vars, const int32_t *e_codes,
                   int32_t *codes, double *log_p);

/* Likelihood findings (Pearl's virtual evidence, "soft evidence") for the NEXT batch call.
 * A finding on variable X is one finite, non-negative weight per state of X; every result of the call is computed from the joint
 * multiplied by the weights of the request's findings:  P(x) * prod_k lambda_k(x_k).  It is what the unmodified reference computes on a
 * network in which every finding variable has an extra binary child V with P(V = 1 | X = x) = lambda(x) / max lambda, observed at 1.
 * It expresses a noisy sensor or a classifier's scores, "X is not x" (weight 0 on x, 1 elsewhere), "X is a or b", a partly trusted label.
 *   Normalised queries: the posterior over the query variables under the weighted joint; scaling a lambda changes nothing.
 *   MIBN_Q_UNNORMALISED: the weighted mass as it is - the caller's lambda is used as given, never rescaled.
 *   mibn_mpe_batch / mibn_map_batch: the maximum is over the weighted joint, log_p is its natural logarithm.
 * A finding variable may be a query or MAP variable; it may not be an evidence variable of the same request, nor be named twice.
 * Finding variables and their ancestors are relevant exactly as evidence variables are; barren descendants are still pruned.  Weights
 * that leave no positive mass behave like impossible evidence: an all-zero posterior, log_p = -inf and codes -1, mass 0.  A single-
 * state variable may carry a finding: a scalar factor, visible in unnormalised and log_p results only.
 * CSR layout: request b has the findings l_vars[l_off[b] .. l_off[b + 1]); finding k has the weights values[v_off[k] .. v_off[k + 1]),
 * exactly card(l_vars[k]) of them (v_off has one entry more than l_vars and is indexed like it).
 * The block is copied.  It belongs to the next batch call and is gone when that call returns, whatever it returns:
 *   mibn_query_batch, mibn_query_batch_ex, mibn_mpe_batch, mibn_map_batch, mibn_bp_batch, mibn_bp_mpe_batch and mibn_bp_evidence_batch consume it; their B must be the block's (MIBN_E_ARG);
 *   mibn_submit_batch and mibn_expect_batch refuse it with MIBN_E_STATE, mibn_posterior_sample_batch with MIBN_E_ARG.
 * A block without a single finding (B = 0 with a call of no requests, or all rows empty) is legal: the call is bit for bit the call
 * without a block.  A call with findings is planned by the host's workers only - no plan templates, no device planner, no adaptive
 * policy -; on the device the weights reach each request's arena through "likelihood_seed_kernel" (a row of its own in
 * mibn_last_kernel_stats), tiny networks answer through "tiny_lh_kernel".
 * Errors, all before anything is enqueued and with the request's index in mibn_last_error: MIBN_E_ARG for a descending l_off, an
 * unknown variable, a variable named twice in a request, a weight vector whose length is not the variable's cardinality, a negative,
 * NaN or infinite weight (here), and for a finding variable that is also evidence of its request (in the call that consumes the block);
 * MIBN_E_STATE before mibn_set_network.
 */
int mibn_set_likelihoods(mibn_t *h, int64_t B, const int64_t *l_off, const int32_t *l_vars,
                         const int64_t *v_off, const double *values);

/*
 * Loopy belief propagation: every single-variable posterior of B requests at once, approximately - sum-product message passing on the
 * factor graph of the CPTs.  Exact on polytrees; on loopy networks an approximation WITHOUT an error bound and without a guarantee of
 * convergence (read `residual`).  Its cost is linear in the network, so it answers where every exact call returns MIBN_E_NOMEM or
 * MIBN_E_LIMIT (a 20 x 20 grid).  Deterministic: no seed, no planner, no per-request program.
 *   Factor graph: one factor per variable v, its CPT, scope S_v = (parents.., v) as mibn_set_network received it, table in C-order.
 *     Every CPT takes part (the MIBN_Q_NOPRUNE rule, as in mibn_mpe_batch).
 *   Edges: e = (f, k) joins factor f and variable u = S_f[k]; numbered by ascending f, then ascending k.  Each carries mu_e (factor ->
 *     variable) and nu_e (variable -> factor), card(u) doubles each.  N(u): the edges of u in ascending edge number.
 *   lambda_u: all ones; one-hot for an evidence variable (all zeros for a code outside the domain, -1 included: not an error);
 *     a likelihood finding's weights as given.
 *   Start: mu_e(x) = 1 / card(u).  Iteration t = 1 .. max_iterations, everything in step t reads step t - 1 only ("flooding"):
 *     1. nu_e(x) = lambda_u(x) * prod over e' in N(u), e' != e, ascending, of mu_e'(x) - no division, CPTs hold zeros -; then every cell
 *        divided by s = the sum over ascending x.
 *     2. mu^_e(x) = sum over the cells c of f with c_k = x, ascending C-order index, of (f[c] times nu_(f,j)(c_j) for ascending j != k);
 *        normalised like 1.
 *     3. mu_e = (1 - damping) * mu^_e + damping * (mu_e of step t - 1); for damping = 0 exactly mu^_e.
 *     4. r_t = max over e, x of |mu_e(x) - its value of step t - 1|; stop after step t if r_t <= tol or t = max_iterations.
 *   Beliefs: b_u(x) ~ lambda_u(x) * prod over e in N(u) of mu_e(x), normalised the same way.
 *   Zero mass - a normalising sum that is 0: impossible evidence, findings that leave nothing -: every belief of the request is 0.0,
 *     iterations[b] the step in which it was seen (0: lambda alone shows it; beliefs: the last step), residual[b] 0.
 *   beliefs[b * sum(card) + (sum of card(w), w < v) + x] = b_v(x), evidence variables included (their one-hot); iterations[b] = steps
 *   executed; residual[b] = the last r_t - the request has converged when it is <= tol.
 * The result of a request is a function of (network, request, max_iterations, tol, damping) alone: bit for bit the same alone or in
 * any batch, at any position, under any chunking (options "chunk", "arena_gb") and in either memory form - a request's messages live
 * in the LDS of its workgroup when they fit in 160 KiB and option "bp_lds" is not 0, else in a slab of the arena; MIBN_E_NOMEM only if
 * a single slab does not fit.
 * Blocking; plans on the calling thread; changes no option and nothing a later call reads; books nothing into the totals.
 * mibn_last_stats / mibn_last_kernel_stats describe it in the row "bp_kernel": launches, HIP-event time, items = requests, and
 * alg_bytes = the bytes of CPT cells read, 8 * (sum over factors of |S_f| * cells(f)) per executed iteration of every request.
 * Consumes a pending mibn_set_likelihoods block (its B must be this call's).
 * Errors, all before anything is enqueued: MIBN_E_ARG for unknown or duplicate evidence variables, a descending e_off, a finding
 * variable that is also evidence of its request, max_iterations < 1, damping outside [0, 1), a negative or NaN tol; MIBN_E_STATE
 * before mibn_set_network; MIBN_E_LIMIT for a cardinality above 255 or 2^31 message cells or more.
 */
int mibn_bp_batch(mibn_t *h, int64_t B, const int64_t *e_off, const int32_t *e_vars, const int32_t *e_codes,
                  int32_t max_iterations, double tol, double damping,
                  double *beliefs /* B * sum(card) */, int32_t *iterations /* B */, double *residual /* B */);

/*
 * Approximate most probable explanation by max-product belief propagation, for B requests at once: one assignment of every variable
 * per request and its log-probability, where mibn_mpe_batch returns MIBN_E_NOMEM or MIBN_E_LIMIT (a 20 x 20 grid).  Exact on
 * polytrees whose maximum is unique; on loopy networks an approximation WITHOUT a bound on the gap to the true maximum and without a
 * guarantee of convergence.  Three things hold always: log_p[b] is the log-probability of the assignment codes[b] itself (score rule
 * below); for fixed other arguments the candidate kept after step t never scores below the one kept after step t - 1, and a polish
 * sweep never lowers the probability of its assignment; when the polish ran fewer than polish_sweeps sweeps, no change of a single
 * variable gives a more probable assignment.  Deterministic: no seed, no planner, no per-request program.
 *   Messages: factor graph, edges, lambda, start, flooding, step 1, damping (step 3), residual and stop rule (step 4) and the zero-mass
 *     rule are word for word those of mibn_bp_batch.  One change, in step 2: mu^_e(x) = the MAXIMUM over the cells c of f with c_k = x,
 *     ascending C-order index, of (f[c] times nu_(f,j)(c_j) for ascending j != k), each product formed in that order, the maximum
 *     started at 0; normalised like 1., by the sum over ascending x.
 *   Max-marginal of u after step t: m_u(x) = lambda_u(x) * prod over e in N(u), ascending, of mu_e(x) (the messages of step t);
 *     normalised by s = the sum over ascending x, and s = 0 is zero mass, seen in step t.
 *   Decode after step t: x^t_u = the lowest state of maximal m_u, for EVERY u, compared on the products before the division (dividing
 *     by s is monotone; it could only merge neighbours).  An evidence variable's lambda is one-hot, so it decodes to its code.
 *   Score of an assignment x: term_v = log f_v[cell of x] + log lambda_v(x_v) (natural logarithm, log 0 = -inf) for every v;
 *     partial_l = the sum of term_v over v = l, l + 64, l + 128, .. ascending; score = the sum of partial_l for l = 0 .. 63 ascending.
 *     The order does not depend on the workgroup size.  -inf is a legal score: the assignment hits a zero of a sparse CPT.
 *   Best so far: the candidate of step 1 is kept; the candidate of a later step replaces it only when its score is strictly
 *     greater.  best_iteration = the step of the kept candidate.  The loop ends by the stop rule of mibn_bp_batch.
 *   Polish (iterated conditional modes) of the kept candidate, after the loop: the moral graph - u and v adjacent when some CPT scope
 *     holds both - is coloured greedily: ascending v, each the smallest colour no already-coloured neighbour has.  A sweep runs over
 *     the colours ascending; every variable v of the colour computes, for every x, L(x) = lambda_v(x) * prod over e in N(v), ascending,
 *     of f_e[the cell of the current assignment with v := x], and moves to the lowest x of maximal L only if L(x) > L(current).
 *     Variables of one colour share no factor: moving them together is moving them in any order.  An evidence variable never moves
 *     (its L is 0 off its code).  The polish stops after a sweep without a move or after polish_sweeps sweeps; sweeps run counts the
 *     last one.  The comparisons are on products, no logarithm: the polish is bit-exact against a host twin.
 *   Result: codes[b * n_vars + v] = the final assignment; log_p[b] = its score, recomputed by the score rule; iterations[b] and
 *     residual[b] as in mibn_bp_batch; info[b * 3 ..] = best_iteration, sweeps run, moves made (info may be NULL).
 *   Zero mass (a normalising sum that is 0, in lambda, a message or a max-marginal): log_p = -inf, code -1 for every non-evidence
 *     variable - evidence variables keep the code they were given -, iterations[b] the step in which it was seen, residual 0, info 0 0 0;
 *     as mibn_mpe_batch does.  A single-state non-evidence variable gets code 0.
 * The result of a request is a function of (network, request, max_iterations, tol, damping, polish_sweeps) alone: bit for bit the same
 * alone or in any batch, at any position, under any chunking (options "chunk", "arena_gb") and in either memory form - the messages
 * and the decoder's state (two code rows, the terms, the 64 partials) live in the LDS of the request's workgroup when together they
 * fit in 160 KiB and option "bp_lds" is not 0, else in a slab of the arena; MIBN_E_NOMEM only if a single slab does not fit.
 * Blocking; plans on the calling thread; changes no option and nothing a later call reads; books nothing into the totals.
 * mibn_last_stats / mibn_last_kernel_stats describe it in the row "bp_max_kernel": launches, HIP-event time, items = requests, and
 * alg_bytes by bp_kernel's rule.  Consumes a pending mibn_set_likelihoods block (its B must be this call's).
 * Errors, all before anything is enqueued: those of mibn_bp_batch, and MIBN_E_ARG for polish_sweeps < 0.
 */
int mibn_bp_mpe_batch(mibn_t *h, int64_t B, const int64_t *e_off, const int32_t *e_vars, const int32_t *e_codes,
                      int32_t max_iterations, double tol, double damping, int32_t polish_sweeps,
                      int32_t *codes /* B * n_vars */, double *log_p /* B */,
                      int32_t *iterations /* B */, double *residual /* B */,
                      int32_t *info /* B * 3 or NULL: best_iteration, sweeps run, moves made */);

/*
 * The Bethe approximation of log P(e) and the belief of every family (a node with its parents) from loopy belief propagation, for B
 * requests at once, with the family beliefs optionally added into expected-count tables - where mibn_query_batch_ex, its P(e) form
 * and mibn_expect_batch return MIBN_E_NOMEM or MIBN_E_LIMIT (a 20 x 20 grid).  log_z[b] estimates log of (P(e) times the findings'
 * weights), as a logarithm: it stays finite where P(e) underflows.  Exact on a polytree once the residual is 0; on a loopy network an
 * approximation WITHOUT a bound and with either sign of error; on a request that did not converge it is the Bethe value of the
 * messages of the last step (read `residual`).  Deterministic: no seed, no planner, no per-request program.
 *   Messages: factor graph, edges, lambda, start, flooding steps 1 to 4, stop rule and zero-mass rule are word for word those of
 *     mibn_bp_batch.  After the loop has ended at step t:
 *   Final phase 1: nu* = step 1 applied once more to the final mu (the messages of step t), with its zero rule.  Everything below
 *     reads the final mu and nu*.
 *   Factor f = f_v: for every cell c in ascending C-order, t_c = f[c] times nu*_(f,j)(c_j) for ascending j, over ALL positions;
 *     Z_f = the sum of t_c over ascending c; the family belief is b_f(c) = t_c / Z_f.
 *   Variable v: Z_v = the sum over ascending x of lambda_v(x) * prod over e in N(v), ascending, of mu_e(x) - the normaliser of the
 *     belief; the beliefs are exactly those of mibn_bp_batch.
 *   Edge e: Z_e = the sum over ascending x of mu_e(x) * nu*_e(x).
 *   Terms: term_v = log Z_(f_v) + log Z_v - log Z_(f_v,0) - log Z_(f_v,1) - .., evaluated left to right over the edges of factor v
 *     in ascending position (natural logarithm).
 *   log_z = the sum of the terms by the score rule of mibn_bp_mpe_batch: partial_l = the sum of term_v over v = l, l + 64, ..
 *     ascending; log_z = the sum of partial_l for l = 0 .. 63 ascending.  The order does not depend on the workgroup size.
 *   Zero mass - any of these normalisers is 0, or a normaliser of the final phase 1 is 0, or the loop saw one: log_z = -inf, every
 *     belief and family belief 0.0, residual 0, iterations[b] the step in which it was seen (the last step for the final phase).
 *   beliefs (may be NULL), iterations, residual: as mibn_bp_batch, byte for byte.
 *   fbeliefs (may be NULL): fbeliefs[b * fcells + foff[v] + c] = b_(f_v)(c), where foff[v] = the sum of the table cells of the factors
 *     below v and fcells their total, c the C-order index in the scope (parents.., v) - the tables back to back, not the pool's layout.
 *   acc (may be NULL; n_acc must be fcells): expected counts, in the layout of a family-belief row.  The call ADDS to what it is given,
 *     as mibn_expect_batch does: for every cell c, acc[c] = acc[c] + weight[b] * b_f(c) for b ascending over the whole call, one
 *     addition after the other (no floating-point atomics).  weight NULL: 1.0 each.  A zero-mass request adds weight * 0.0.
 * The result - acc included - is a function of (network, the requests in their order, max_iterations, tol, damping, weight) alone: bit
 * for bit the same under any chunking (options "chunk", "arena_gb") and in either memory form; a request's log_z, beliefs and family
 * beliefs are the same alone or in any batch, at any position.  A request's messages, Z_f, terms and partials live in the LDS of its
 * workgroup when together they fit in 160 KiB and option "bp_lds" is not 0, else in a slab of the arena.  With fbeliefs or acc the
 * launch's family beliefs are kept in the arena too, one row per request behind the slabs; a launch holds as many requests as "chunk" allows and as
 * have a slab (second form) plus such a row in the "arena_gb" budget; MIBN_E_NOMEM only if one request does not fit.
 * Blocking; plans on the calling thread; changes no option and nothing a later call reads; books nothing into the totals.
 * mibn_last_stats / mibn_last_kernel_stats describe it in the row "bp_evidence_kernel": launches, HIP-event time, items = requests,
 * and alg_bytes by bp_kernel's rule plus one more pass over the CPT cells, 8 * fcells, per request; with acc a second row,
 * "bp_accumulate_kernel", one launch after each of the first (alg_bytes = 8 * fcells * (requests of the launch + 2)).
 * Consumes a pending mibn_set_likelihoods block (its B must be this call's).
 * Errors, all before anything is enqueued: those of mibn_bp_batch, and MIBN_E_ARG for n_acc != fcells when acc is given and for a
 * negative, NaN or infinite weight.
 */
int mibn_bp_evidence_batch(mibn_t *h, int64_t B, const int64_t *e_off, const int32_t *e_vars, const int32_t *e_codes,
                           int32_t max_iterations, double tol, double damping,
                           const double *weight /* B or NULL */, double *log_z /* B */,
                           double *beliefs /* B * sum(card) or NULL */, double *fbeliefs /* B * fcells or NULL */,
                           int64_t n_acc, double *acc /* fcells, in/out, or NULL */,
                           int32_t *iterations /* B */, double *residual /* B */);

/* Statistics of the last mibn_query_batch call (for the roofline report). */
typedef struct mibn_stats {
    double alg_bytes;      /* sum over steps of 8*(sum input cells + output cells) */
    double alg_flops;      /* sum over steps of n_inputs * product-scope cells */
    double n_steps;        /* elimination + final product steps executed */
    double kernel_ms;      /* HIP-event time of all kernel launches (sum over launches) */
    double plan_ms;        /* host planning wall time */
    double h2d_ms;         /* program upload */
    double d2h_ms;         /* result download */
    double total_ms;       /* whole call, host wall clock */
    double n_launches;     /* kernel launches */
    double arena_bytes;    /* device scratch arena in use */
    double max_step_cells; /* largest product scope of any step */
    double n_workgroups;   /* work items (= workgroups) launched */
} mibn_stats;
int mibn_last_stats(const mibn_t *h, mibn_stats *out);

/* Per-kernel breakdown of the last mibn_query_batch call: HIP-event time on the library's stream and
 * the section-8(d) algorithmic bytes of the steps each kernel executed (tiles pro rata).  Fills at most
 * `cap` entries (one per kernel that ran), *n = number filled. */
typedef struct mibn_kernel_stat {
    char name[48];
    double launches, ms, alg_bytes, items;
} mibn_kernel_stat;
int mibn_last_kernel_stats(const mibn_t *h, int32_t cap, mibn_kernel_stat *out, int32_t *n);

/*
 * Asynchronous form of mibn_query_batch for streams of batches: mibn_submit_batch plans, uploads and launches and
 * returns at once with a ticket; mibn_wait(ticket) blocks until that call's posteriors are in `out` (which must
 * stay valid until then).  Up to two calls may be in flight, so the host plans call s+1 while the GPU still runs
 * call s.  mibn_drain waits for every launch and books its time; mibn_total_stats / mibn_total_kernel_stats are
 * the counters of mibn_last_stats / mibn_last_kernel_stats accumulated since the context was created (differences
 * over a region of calls are what bench.py reports).
 */
int mibn_submit_batch(mibn_t *h, int64_t B, const int64_t *q_off, const int32_t *q_vars,
                      const int64_t *e_off, const int32_t *e_vars, const int32_t *e_codes,
                      const int64_t *out_off, double *out, int32_t *ticket);
int mibn_wait(mibn_t *h, int32_t ticket);
int mibn_drain(mibn_t *h);
int mibn_total_stats(const mibn_t *h, mibn_stats *out);
int mibn_total_kernel_stats(const mibn_t *h, int32_t cap, mibn_kernel_stat *out, int32_t *n);

/* Plan only (no device work): fills alg_bytes / alg_flops / n_steps / max_step_cells for one
 * request.  Also usable without a device through a context created by mibn_create_planner(). */
int mibn_plan_stats(mibn_t *h, int32_t n_q, const int32_t *q_vars, int32_t n_e,
                    const int32_t *e_vars, mibn_stats *out);
int mibn_create_planner(mibn_t **out); /* host-only context: set_network/plan_stats work, queries fail */

/* The elimination order the planner executes for one request: order[0 .. *n) = hidden variables, first eliminated
 * first (`order` must hold n_vars entries).  The reference eliminates in Python-set iteration order (bayes_net.py:766,
 * 779); tests hand this order to the CPU oracle so that it can answer the wide requests in seconds instead of minutes. */
int mibn_plan_order(mibn_t *h, int32_t n_q, const int32_t *q_vars, int32_t n_e, const int32_t *e_vars,
                    int32_t *order, int32_t *n);

/* Cheap per-request cost estimate for shard balancing ("balance by the planner's bytes_query, not
 * by count - per-request cost varies 1000x"): cost[b] = section-8(d) bytes of the cheaper of the planner's two sweep
 * orders for request b (no program is emitted, no min-fill search; ~2 us per request and planner thread).  Works on a
 * planner-only context too.  `sorobn_amd.sharding.cost_balanced_ranges` turns the prefix sums into contiguous shards. */
int mibn_estimate_costs(mibn_t *h, int64_t B, const int64_t *q_off, const int32_t *q_vars, const int64_t *e_off,
                        const int32_t *e_vars, double *cost);

/* Wait for everything this context has submitted to its device (kernels, copies, collectives). */
int mibn_device_synchronize(mibn_t *h);

/* Tunables: "arena_gb" (scratch budget), "threads" (planner threads), "chunk" (requests per planning /
 * launch chunk), "plan_cache" (0: plan every request, no plan templates for repeated request shapes), "adaptive" (1: when host planning rather than the GPU bounds a stream
 * of calls, move the elimination-order search to the device - "gpu_search" - or, for networks of more than 128 variables,
 * reserve the min-fill search for ever more expensive requests; given back when the host has slack), "gpu_search" (1: the
 * order search of every chunk but the first of a call runs as a kernel, one request per lane, the same code as on the
 * host: identical orders and programs; 2: every chunk, synchronously - tests), "minfill_above" (bytes of the best sweep order above which the min-fill search runs), "stagger" (groups
 * of requests whose levels are staggered inside a chunk), "tiny" (0: never use the
 * small-network kernel - one lane per request, CPTs in LDS, no planning - that answers blocking calls on networks of at
 * most 32 variables / 4096 CPT cells / 65536 joint states), "sweep" (0..5: the most four-state variables of one big table
 * a single pass may eliminate with the tile resident in LDS - ve_sweep_kernel; below 3: off), "sweep_iters" (tiles per
 * workgroup of that kernel; "sweep_adapt": fewer - down to 2 - in launches of fewer workgroups than this, 0 = off),
 * "order_weights" (0: compare candidate elimination orders by plain section-8(d) bytes instead of the class-weighted
 * model), "order_effort" (default 1: more candidate orders, and the byte model's best two both emitted where the best costs
 * more than "second_above" modelled bytes - the program that moves fewer bytes stays; 0: round 5's search; calls the device
 * plans skip the second emission unless "second_on_device" is 1), "builtin_sweeps" (1: two depth-first topological orders as additional candidates), "streams" (2: consecutive chunks of a call run concurrently on two streams with an arena each), "first_chunk" (short first chunk of a call: 0 never, 1 when the GPU is idle, 2 always).
 * Test and profiling hooks: "sweep_canon" (0: the sweep kernel's general path for every step), "small_cells", "big_iters", "tile_h", "fuse", "chain", "outer" (force the
 * kernels' step forms onto small networks), "split_kinds" (one launch per class of work and level, so that
 * mibn_last_kernel_stats reports per-class rates), "trace" (one stderr line per launch), "gibbs_lds" (0: the Gibbs
 * kernel reads the CPTs through L2 even when they would fit in LDS), "bp_lds" (default 1; 0: mibn_bp_batch keeps the messages in slabs
 * of the arena even when they would fit in LDS). */
int mibn_set_option(mibn_t *h, const char *name, double value);

/*
 * Gibbs sampling (replaces BayesNet._gibbs_sampling, bayes_net.py:665-737): n_chains independent
 * chains of n_iterations single-site updates each (the reference's n_iterations counts single-site
 * updates, bayes_net.py:720-733; every iteration is recorded, no burn-in, no thinning).
 *   cycle     update order: every non-evidence variable exactly once (the reference cycles through
 *             sorted(nodes - event), bayes_net.py:697,718); NULL = ascending variable id
 *   counts[prod card(q_vars)]   int64 histogram over the joint query state (C-order over q_vars,
 *             last fastest), summed over all chains and iterations; the estimate of the reference
 *             (bayes_net.py:736-737) is counts / (n_chains * n_iterations)
 * Random stream: counter-based Philox4x32-10 keyed by (seed, chain); parity with the reference's stream
 * is unpinned (it depends on the third-party `vose` sampler, see oracle/README.md); our own stream is pinned by
 * tests/sample_check.py.
 */
int mibn_gibbs(mibn_t *h, int32_t n_q, const int32_t *q_vars, int32_t n_e, const int32_t *e_vars,
               const int32_t *e_codes, const int32_t *cycle, int64_t n_chains, int64_t n_iterations,
               uint64_t seed, int64_t *counts);

/* A shard of the chains of one mibn_gibbs call: chains [chain_first, chain_first + n_chains) of the stream `seed` (the
 * Philox key is (seed, global chain index), so the union of disjoint shards - on any number of GPUs - gives bit for bit
 * the histogram of the unsharded call; mibn_gibbs == chain_first 0).  Multi-GPU: every rank runs its chain range and the
 * int64 histograms are summed with mibn_comm_reduce_i64. */
int mibn_gibbs_shard(mibn_t *h, int32_t n_q, const int32_t *q_vars, int32_t n_e, const int32_t *e_vars,
                     const int32_t *e_codes, const int32_t *cycle, int64_t chain_first, int64_t n_chains,
                     int64_t n_iterations, uint64_t seed, int64_t *counts);

/* Parity hook for the deterministic half of the Gibbs path (tests): the Markov-blanket conditionals the chain samples from,
 * bayes_net.py:699-710 - pointwise_mul of the CPTs of a node and its children, normalised per boundary configuration.  For each
 * of n_rows full joint states (states[row * n_vars + v] = label code; evidence entries are overwritten by e_codes) out[row *
 * card(var) + x] = P(var = x | the rest of the row), computed by gibbs_kernel ITSELF: the same update programs, the same
 * LDS-resident tables and the same one of its three update forms a mibn_gibbs call with this network / evidence / cycle and
 * n_rows chains takes - the weights are written out, normalised, where the chain would draw from them.  Only the random
 * stream of the Gibbs path stays unpinned (the reference's depends on the absent third-party `vose` sampler). */
int mibn_gibbs_conditional(mibn_t *h, int32_t n_e, const int32_t *e_vars, const int32_t *e_codes, const int32_t *cycle,
                           int32_t var, int64_t n_rows, const uint8_t *states, double *out);

/*
 * Forward (ancestral) sampling and the two approximate algorithms built on it.
 *   mibn_sample          BayesNet.sample(n, init) / _forward_sample (bayes_net.py:518-575): n_samples joint samples,
 *                        states[sample * n_vars + v] = label code of variable v; `init` variables are clamped
 *   mibn_sampling_query  mode MIBN_REJECTION = _rejection_sampling (577-619): counts[cell] = samples that agree with
 *                        the event, per joint query state; mode MIBN_LIKELIHOOD = _llh_weighting (621-663): the event
 *                        is clamped, weight_sum[cell] = sum of the sample likelihoods (the product of P(value |
 *                        parents) over ALL nodes, as the reference computes it) and counts[cell] = samples per state;
 *                        the reference's answer is (weight_sum / counts) normalised
 * Random stream: Philox4x32-10 keyed by (seed, sample, variable); parity with the reference's stream is unpinned,
 * our own stream is pinned by tests/sample_check.py (see mibn_gibbs).
 */
#define MIBN_REJECTION 1
#define MIBN_LIKELIHOOD 2
int mibn_sample(mibn_t *h, int64_t n_samples, int32_t n_init, const int32_t *init_vars, const int32_t *init_codes,
                uint64_t seed, uint8_t *states);
int mibn_sampling_query(mibn_t *h, int32_t mode, int32_t n_q, const int32_t *q_vars, int32_t n_e, const int32_t *e_vars,
                        const int32_t *e_codes, int64_t n_samples, uint64_t seed, double *weight_sum, int64_t *counts);

/* Parity hook for the deterministic half of the sampling paths (tests): sample_kernel ITSELF walks n_rows GIVEN joint states
 * (states[row * n_vars + v] = label code) exactly as it walks a sample it draws - same CPT offsets, same row sums, same running
 * sums, same likelihood product - and writes them out instead of drawing from them:
 *   likelihood[row]                        the product of P(state_v | parents in the state) over ALL nodes, the weight
 *                                          _forward_sample hands to _llh_weighting (bayes_net.py:541-546, 646-652)
 *   cdf[(row * n_vars + v) * cdf_stride + x]   x < card(v): the running sum of the conditional row P(v = . | parents in the state)
 *                                          the inverse-CDF draw of v compares u * total with (total = the entry at card(v) - 1) -
 *                                          the weights the reference hands to its alias sampler (bayes_net.py:28-42, 530-539)
 * Only the random stream of the sampling paths stays unpinned (the reference's depends on the absent third-party `vose`). */
int mibn_sample_probe(mibn_t *h, int64_t n_rows, const uint8_t *states, int32_t cdf_stride, double *likelihood, double *cdf);

/*
 * Grouped counting of label codes: the `X.groupby([*parents, node]).size()` of
 * BayesNet.partial_fit (bayes_net.py:467-510) and the pairwise `X.groupby([u, v]).size()` of structure.chow_liu
 * (structure.py:33-45).  No network needed.
 *   codes[n_cols * n_rows]    label codes, code < card[col] <= 256; row_major = 0: codes[col * n_rows + row],
 *                             row_major = 1: codes[row * n_cols + col] (what DataFrame.to_numpy() gives; transposed on
 *                             the device)
 *   scope_off[n_tables + 1], scope_cols[]   CSR: the columns of table t
 *   counts_off[n_tables + 1], counts[]      dense C-order contingency table of every table (last column fastest);
 *                             tables of up to 16384 cells are counted in LDS histograms, larger ones (up to 2^28
 *                             cells) with global atomics
 */
int mibn_count_tables(mibn_t *h, int64_t n_rows, int32_t n_cols, const uint8_t *codes, int32_t row_major, const int32_t *card,
                      int32_t n_tables, const int64_t *scope_off, const int32_t *scope_cols, const int64_t *counts_off,
                      int64_t *counts);

/*
 * Score-based structure learning: a data set kept on the device and decomposable family scores computed there (an extension: the
 * reference learns no structure but the Chow-Liu tree).  No network needed; a context may hold several data sets.
 *
 * mibn_dataset_create uploads the code matrix once (layout and limits of mibn_count_tables: row_major input is transposed on the
 * device, cardinalities 1..256 or MIBN_E_LIMIT; a code >= card[col] is MIBN_E_ARG, MIBN_E_HIP if the allocation fails) and keeps it,
 * with `card`, under *id.  mibn_dataset_destroy frees it; mibn_destroy frees what is left.  A destroyed or unknown id is MIBN_E_ARG.
 *
 * mibn_score_families: family f is scope_cols[scope_off[f] .. scope_off[f + 1]), parents first, CHILD LAST (at least the child, no
 * column twice); scores[f] = its score of `kind` in natural logs.  With q = the product of the parents' cardinalities (1 without
 * parents; the cardinalities are the data set's, whether or not every label combination occurs), r = card(child), N = n_rows, N_jk
 * the count of child state k under parent configuration j and N_j = sum_k N_jk:
 *   MIBN_SCORE_LOGLIK  LL = sum over cells with N_jk > 0 of N_jk * (ln N_jk - ln N_j)
 *   MIBN_SCORE_BIC     LL - 0.5 * ln(max(N, 1)) * q * (r - 1)
 *   MIBN_SCORE_AIC     LL - q * (r - 1)
 *   MIBN_SCORE_BDEU    sum_j [lgamma(a/q) - lgamma(a/q + N_j)] + sum_jk [lgamma(a/(q r) + N_jk) - lgamma(a/(q r))], a = ess > 0
 *   MIBN_SCORE_K2      sum_j [lgamma(r) - lgamma(r + N_j)] + sum_jk lgamma(1 + N_jk)
 * (`ess` is read by MIBN_SCORE_BDEU only).  Empty configurations and empty cells contribute exactly 0.  The tables (at most 2^28
 * cells each) are counted by the kernels of mibn_count_tables into a device buffer and reduced there; a call is cut into sub-batches
 * by the cell budget of that buffer (option score_cells) - the caller sees one call.  The addition order depends on the shape of a
 * family's table alone: the same family on the same rows gives the same bits in any call, alone or among others, through any handle.
 * Blocking; validated on the host before anything is launched; writes no option or policy state; its kernels are booked in the
 * last-call statistics only (entries count_kernel and score_kernel of mibn_last_kernel_stats).
 */
#define MIBN_SCORE_LOGLIK 0
#define MIBN_SCORE_BIC 1
#define MIBN_SCORE_AIC 2
#define MIBN_SCORE_BDEU 3
#define MIBN_SCORE_K2 4
int mibn_dataset_create(mibn_t *h, int64_t n_rows, int32_t n_cols, const uint8_t *codes, int32_t row_major, const int32_t *card,
                        int32_t *id);
int mibn_dataset_destroy(mibn_t *h, int32_t id);
int mibn_score_families(mibn_t *h, int32_t id, int32_t kind, double ess, int32_t n_fam, const int64_t *scope_off,
                        const int32_t *scope_cols, double *scores);

/*
 * Constraint-based structure learning: conditional-independence tests of X and Y given Z_1 .. Z_m on a resident data set (an
 * extension, as the scores above).  Test t is scope_cols[scope_off[t] .. scope_off[t + 1]): the m >= 0 conditioning columns first,
 * then X, then Y LAST (at least two columns, none twice).  With q = the product of the conditioning cardinalities (1 without),
 * N_xyz the count of (x, y) in stratum z, N_xz and N_yz its row and column sums and N_z its total:
 *   MIBN_CI_G2   stat = 2 * sum over cells with N_xyz > 0 of N_xyz * ln((N_xyz * N_z) / (N_xz * N_yz))
 *   MIBN_CI_X2   stat = sum over cells with N_xz * N_yz > 0 of (N_xyz * N_z - N_xz * N_yz)^2 / (N_z * N_xz * N_yz)
 *   adj_dof[t]   = sum over strata with N_z > 0 of (rows with N_xz > 0 - 1) * (columns with N_yz > 0 - 1), an exact integer
 * (the classic degrees of freedom, q * (card(X) - 1) * (card(Y) - 1), need no device).  Empty strata, rows and columns contribute
 * exactly 0; an exactly independent table has X2 exactly 0; a data set of zero rows gives stat 0 and adj_dof 0.  A table above 2^28
 * cells and a data set of 2^31 rows or more are MIBN_E_LIMIT; an unknown kind, id or column, a column twice and a test of fewer than
 * two columns are MIBN_E_ARG.  Counting, sub-batches (option score_cells), blocking, validation and statistics are those of
 * mibn_score_families (entries count_kernel and citest_kernel of mibn_last_kernel_stats); the addition order depends on the shape
 * (q, card(X), card(Y)) of a test's table alone, so the same test on the same rows gives the same bits in any call.
 */
#define MIBN_CI_G2 0
#define MIBN_CI_X2 1
int mibn_ci_tests(mibn_t *h, int32_t id, int32_t kind, int32_t n_tests, const int64_t *scope_off, const int32_t *scope_cols,
                  double *stat, int64_t *adj_dof);

/*
 * Integer row weights on the counting path: aggregated data (one row per pattern plus a frequency) and bootstrap resamples (a
 * resample of N rows IS a vector of N multiplicities summing to N) without expanding the rows.  A weight set is uint32[n_rows]; a
 * table counted under set s is the contingency table with row i counted w_s[i] times, an exact integer whatever the launch
 * geometry.  Every call below gives, bit for bit, what its unweighted twin gives on the rows written out w_s[i] times each.
 *
 * mibn_dataset_set_weights replaces the weight sets of a resident data set by weights[n_sets * n_rows], set-major (set s is
 * weights[s * n_rows .. (s + 1) * n_rows)); n_sets = 0 drops them (weights may then be NULL).  W_s, the sum of set s, must be at
 * most 2^32 - 1, else MIBN_E_LIMIT (checked on the host; no partial sum of a workgroup's 32-bit histogram can then overflow).  On
 * any error the data set keeps the sets it had.
 *
 * mibn_dataset_bootstrap replaces the weight sets by n_sets multinomial resamples drawn on the device.  The rule: for set s and
 * draw j = 0 .. n_rows - 1, u = the Philox4x32-10 uniform of mibn_sample's convention with counter (j_lo, j_hi, s, 0) and key
 * ((uint32) seed, (uint32)(seed >> 32) ^ 0x85EBCA6B) - 53 bits of the first two output words, a double in [0, 1) -; the drawn row
 * is min(floor(u * n_rows), n_rows - 1), the product formed in fp64; its weight goes up by one.  Set s is a function of
 * (seed, s, n_rows) alone, not of n_sets, and every W_s = n_rows.  weights_out (n_sets * n_rows, or NULL) receives the sets.  A data
 * set of more than 2^32 - 1 rows is MIBN_E_LIMIT.
 *
 * mibn_score_families_w / mibn_ci_tests_w: mibn_score_families / mibn_ci_tests with one weight-set index per table, wset[t] in
 * [-1, n_sets) (else MIBN_E_ARG); -1 = every row once.  N of the BIC penalty and of the zero-row rules is W_s (n_rows for -1);
 * mibn_ci_tests_w refuses a table whose N is 2^31 or more (MIBN_E_LIMIT).  The reduction is that of the unweighted calls on the
 * counted tables (the families of a sub-batch are reduced N by N: one launch set per distinct N, one for a bootstrap); sub-batches
 * (option score_cells), blocking, validation before any launch and statistics are theirs too, the counting booked under
 * count_weighted_kernel (alg_bytes = codes read + 4 * n_rows per table + the tables) instead of count_kernel.
 *
 * mibn_count_tables_w: mibn_count_tables with one weight vector weights[n_rows] (sum at most 2^32 - 1, else MIBN_E_LIMIT).
 */
int mibn_dataset_set_weights(mibn_t *h, int32_t id, int32_t n_sets, const uint32_t *weights /* n_sets x n_rows, set-major */);
int mibn_dataset_bootstrap(mibn_t *h, int32_t id, int32_t n_sets, uint64_t seed, uint32_t *weights_out /* n_sets x n_rows or NULL */);
int mibn_score_families_w(mibn_t *h, int32_t id, int32_t kind, double ess, int32_t n_fam, const int64_t *scope_off,
                          const int32_t *scope_cols, const int32_t *wset /* n_fam */, double *scores);
int mibn_ci_tests_w(mibn_t *h, int32_t id, int32_t kind, int32_t n_tests, const int64_t *scope_off, const int32_t *scope_cols,
                    const int32_t *wset /* n_tests */, double *stat, int64_t *adj_dof);
int mibn_count_tables_w(mibn_t *h, int64_t n_rows, int32_t n_cols, const uint8_t *codes, int32_t row_major, const int32_t *card,
                        int32_t n_tables, const int64_t *scope_off, const int32_t *scope_cols, const int64_t *counts_off,
                        const uint32_t *weights /* n_rows */, int64_t *counts);

/*
 * Exact structure learning: the best-scoring DAG under a decomposable score, by dynamic programming over variable subsets
 * (Silander and Myllymaki 2006; Koivisto and Sood 2004).  The call takes no network and no data set - its input is a list of local
 * scores, e.g. those of mibn_score_families or mibn_score_families_w, unchanged.
 *
 * Candidates.  Candidate f says: child fam_child[f] may take exactly the parent set fam_parents[f] (bit u = column u is a parent)
 * at score fam_score[f].  A child's parent set is always one of its candidates; a set that is not listed is not allowed - limits on
 * the number of parents, required and forbidden edges are expressed by what is listed.
 *
 * Validation, on the host before any launch.  MIBN_E_ARG: n_vars < 1, a child outside [0, n_vars), a parent bit at or above n_vars
 * or the child's own bit, a non-finite score (NaN, +-inf), the same (child, parent set) listed twice.  MIBN_E_LIMIT: n_vars above
 * MIBN_BEST_DAG_MAX_VARS (the tables take 12 n 2^(n-1) + 9 2^n bytes: 2.6 GB at 24).  MIBN_E_HIP if their allocation fails.
 *
 * Phase A, best parent sets.  For child v and every C inside V \ {v}: bps[v][C] = the best candidate (score, parent mask) of v with
 * parents inside C, "best" being the maximum of one TOTAL order: the higher score first; at equal score (==) the smaller mask as an
 * unsigned integer.  The winner's pair is kept whole, score bits and mask together; without such a candidate the entry is
 * (-inf, 0xFFFFFFFF).  The order being total, the table is a function of the candidate list alone, whatever schedule computed it.
 *
 * Phase B, sinks.  best[{}] = 0; best[S] = max over v in S of (best[S \ {v}] + bps[v][S \ {v}].score) - one fp64 addition per
 * term, the terms compared in ascending v with a strict > starting from -inf, so that ties go to the smallest v.  sink[S] is that v,
 * or 255 if every term is -inf.
 *
 * Traceback.  From S = V: v = sink[S], parents_out[v] = bps[v][S \ {v}].mask, S = S \ {v}, n_vars times.  order_out is a
 * topological order, roots first: the reverse of the sinks peeled.  total_out = best[V], that nested sum - equal to the sum of the
 * chosen candidates' scores only up to rounding.  No DAG possible from the candidates (best[V] = -inf): MIBN_OK with total_out =
 * -inf, every parents_out[v] = 0xFFFFFFFF and every order_out[v] = -1.
 *
 * Blocking.  Writes no option or policy state; bit-for-bit repeatable in any call and through any handle (the options
 * dag_tile_bits / dag_group_bits - test hooks that shape phase A's passes - change no bit).  Last-call statistics only: the row
 * dag_subset_kernel is the fill, the scatter of the candidates and the passes of phase A (alg_bytes: entries read and written),
 * dag_sink_kernel the n_vars + 1 levels of phase B and the traceback.
 */
#define MIBN_BEST_DAG_MAX_VARS 24
int mibn_best_dag(mibn_t *h, int32_t n_vars, int64_t n_fam, const int32_t *fam_child, const uint32_t *fam_parents /* bit u = column u is a parent */,
                  const double *fam_score, uint32_t *parents_out /* n_vars */, int32_t *order_out /* n_vars */, double *total_out);

/*
 * Exact Bayesian arc posteriors: the posterior probability of every candidate parent set and of every arc, averaged over ALL
 * DAGs, by the sum-product form of the same subset DP (Koivisto and Sood 2004; Koivisto 2006).  Input and validation are
 * mibn_best_dag's - the same candidates, the same rules and error codes; MIBN_E_LIMIT above MIBN_ARC_POSTERIOR_MAX_VARS (the
 * tables take 8 n 2^(n-1) + 16 2^n bytes: 1.9 GB at 24).  The scores are log weights: with log marginal likelihoods (bdeu, k2)
 * the results are Bayesian posteriors.
 *
 * The prior.  The results are posteriors under an ORDER-MODULAR prior: the sum runs over pairs (linear order, parent sets
 * consistent with it), so a DAG weighs its number of linear extensions times prod exp(score) - NOT uniform over DAGs.  At
 * n_vars = 2 with every candidate listed the empty graph counts twice, each one-arc graph once.
 *
 * Arithmetic.  Everything is a natural logarithm in fp64.  a (+) b = m + log1p(exp(-|a - b|)) with m = max(a, b), and m itself
 * when m = -inf or the other operand is -inf: a single term passes through bit for bit, no NaN can form.
 *
 * Centring.  c_v = the maximum score among child v's candidates, 0 if it has none; the DP runs on s' = s - c_v (one fp64
 * subtraction).  The posteriors do not depend on c_v; the rounding errors scale with the magnitudes that are left.
 *
 * Subset sums.  For child v and every C inside V \ {v}: alpha_v(C) = (+) over the candidates P of v inside C of s'_v(P), -inf
 * without one - one step per index bit b of the child's table, entry[i | 1 << b] = entry[i | 1 << b] (+) entry[i], the bits in
 * the order of the pass schedule (mibn_best_dag's; the options dag_tile_bits / dag_group_bits shape it).
 *
 * Forward and backward.  L({}) = R({}) = 0; L(S) = (+) over v in S of (L(S \ v) + alpha_v(S \ v)); R(T) = (+) over v in T of
 * (alpha_v(V \ T) + R(T \ v)) - the terms folded in ascending v from -inf.  L(V) = R(V) up to rounding; L(V) is the one used.
 * log_evidence_out = L(V) + c_0 + c_1 + .., the c_v added one by one in ascending v.
 *
 * Gaps.  For S inside V \ {v}: g_v(S) = L(S) + R(V \ S \ {v}); Gamma_v(P) = (+) over S with P inside S inside V \ {v} of g_v(S) -
 * one step per index bit, entry[i] = entry[i] (+) entry[i | 1 << b], in the order of the same schedule.
 *
 * Outputs.  log_post_out[f] = (s'_f + Gamma_v(P_f)) - L(V): the log posterior that child v has exactly the parent set P_f; over
 * one child's candidates the exp of these sums to 1.  arc_out[u * n_vars + v] = sum over the candidates f of child v with u in P_f
 * of exp(log_post_out[f]) - a linear sum in ONE order, a function of the candidate list alone (no floating-point atomics): the
 * list is cut into segments of 65 536 consecutive candidates; within a segment lane t of 256 adds its candidates first + t,
 * first + t + 256, .. in ascending f starting from 0.0; the 256 lanes are folded in a tree, lane[t] += lane[t + h] for h = 128,
 * 64, .., 1; the segments' results are added in ascending order starting from 0.0.
 *
 * No candidate structure (L(V) = -inf): MIBN_OK with log_evidence_out = -inf, every log_post_out = -inf and every arc 0.
 *
 * Accuracy.  A sum has no total order behind it: unlike mibn_best_dag's, these results are NOT schedule-independent in their
 * last bits - the order in which the index bits are taken is part of the value.  Under fixed options a call is bit-for-bit
 * repeatable, in any call and through any handle; across schedules (the options dag_tile_bits / dag_group_bits) - and against a
 * twin that uses another exp / log1p - the results agree within 8 D 2^-53 (1 + M), D = n^2 + 2 n + ceil(log2(n_fam + 1)) the
 * depth of roundings and M the largest finite magnitude among L, R and the centred scores: absolute on log_post and
 * log_evidence, and on the arcs as probabilities.  (The schedules of today all take the bits in ascending order, whatever the
 * tiling, which gives every entry the same chain of operations; that is a property of this planner, not of the contract.)
 *
 * Blocking.  Writes no option or policy state.  Last-call statistics only: dag_post_subset_kernel is the fill, the scatter and
 * the passes of the subset sum, dag_post_level_kernel the n_vars + 1 levels of L and R, dag_post_superset_kernel the passes of
 * the superset sum, dag_post_arc_kernel the candidate kernel and the two kernels of the arc sums.
 */
#define MIBN_ARC_POSTERIOR_MAX_VARS 24
int mibn_arc_posteriors(mibn_t *h, int32_t n_vars, int64_t n_fam, const int32_t *fam_child, const uint32_t *fam_parents /* bit u = column u is a parent */,
                        const double *fam_score, double *log_post_out /* n_fam */, double *arc_out /* n_vars x n_vars, row = from */,
                        double *log_evidence_out);

/*
 * Multi-GPU: one process per GPU, requests / chains sharded with no data-path collective; the
 * only communication is the final gather of the posteriors (exact path) or the sum of the histograms (Gibbs).  These
 * entry points sit directly on RCCL (librccl.so is dlopen'ed by mibn_comm_init - a single-GPU process never loads it) and
 * run on a stream of their own (the gather of batch s must not queue behind the kernels of batch s + 1), over xGMI between the GPUs of a node.  No PyTorch involved.
 *   mibn_comm_probe       loads librccl.so and resolves its entry points, nothing else: what can fail on one rank alone is
 *                         checked on EVERY rank before anybody enters the collective init
 *   mibn_comm_unique_id   rank 0 (only) creates the 128-byte RCCL id; the caller hands it to the other ranks out of band
 *                         (sorobn_amd/sharding.py: a file next to the rendezvous port, single node)
 *   mibn_comm_init        collective: every rank calls it with the same id.  Bounded: a rank that has waited
 *                         MIBN_COMM_INIT_TIMEOUT_S seconds (environment, default 180) for the others returns MIBN_E_COMM with
 *                         a message naming the likely causes instead of hanging the launch
 *   mibn_device_info      one text line about this context's device (name, PCI bus id, link type / hops to every other
 *                         visible device) for the launch log
 *   mibn_comm_count       ncclCommCount / ncclCommUserRank of the live communicator: what RCCL itself reports, for the
 *                         bench line of an N > 1 run (`config.rccl_ranks`)
 *   mibn_comm_allgather_f64   recv[r * n .. (r+1) * n) = rank r's send[0 .. n)   (host buffers, staged through HBM)
 *   mibn_comm_reduce_i64      sum over ranks of buf[0 .. n) -> buf on `root` (other ranks' buf unchanged)
 *   mibn_comm_allreduce_max_f64   element-wise max over ranks, in place (the bench's max-over-ranks step time)
 *   mibn_comm_barrier     all ranks have reached the call and their device work is complete
 */
#define MIBN_COMM_ID_BYTES 128
int mibn_comm_probe(mibn_t *h);
int mibn_device_info(mibn_t *h, char *buf, int32_t cap);
int mibn_comm_unique_id(mibn_t *h, void *id_out /* MIBN_COMM_ID_BYTES */);
int mibn_comm_init(mibn_t *h, int32_t rank, int32_t world, const void *id /* MIBN_COMM_ID_BYTES */);
int mibn_comm_count(mibn_t *h, int32_t *n_ranks, int32_t *my_rank);
int mibn_comm_destroy(mibn_t *h);
int mibn_comm_allgather_f64(mibn_t *h, const double *send, int64_t n, double *recv);
int mibn_comm_reduce_i64(mibn_t *h, int64_t *buf, int64_t n, int32_t root);
int mibn_comm_allreduce_max_f64(mibn_t *h, double *buf, int64_t n);
int mibn_comm_barrier(mibn_t *h);

#ifdef __cplusplus
}
#endif
#endif /* MIBN_H */
