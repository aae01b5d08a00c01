/*
 * moeva_mi355x.h -- C ABI of the MI355X-native MoEvA2 engine (libmoeva_mi355x.so).
 *
 * The reference is pure Python: its hot path is reached through
 *   Moeva2.generate(x, minimize_class)             src/attacks/moeva2/moeva2.py:174-207
 *   DefaultProblem._evaluate(x, out)               src/attacks/moeva2/default_problem.py:99-140
 * and, inside pymoo 0.4.2.2 (not vendored), R-NSGA-III survival + mating.  Each entry
 * point below replaces one of those surfaces; the Python host package
 * (moeva2_amd.attacks.moeva2.*) binds them with ctypes exactly as a maintainer would add
 * to the reference.
 *
 * Conventions
 *  - status codes (MV_OK == 0); mv_last_error() returns a thread-local message;
 *  - no exceptions cross the ABI; no torch types; plain pointers and sizes;
 *  - pointers documented "dev" are device (HBM) pointers owned by the caller
 *    (e.g. torch tensors' data_ptr()); "host" pointers are read synchronously;
 *  - every launch is ordered on the caller's hipStream_t (passed as void*; NULL = default
 *    stream) and is asynchronous unless stated;
 *  - one mv_engine per (device, problem); an engine is thread-compatible, not thread-safe.
 */
#ifndef MOEVA_MI355X_H
#define MOEVA_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  MV_OK = 0,
  MV_ERR_ARG = 1,   /* invalid argument / shape */
  MV_ERR_HIP = 2,   /* HIP runtime error */
  MV_ERR_STATE = 3, /* call out of order (e.g. no states bound) */
};

/* gene kinds (feature_encoder.py:169-181 get_type_mask_genetic) */
enum { MV_GENE_REAL = 0, MV_GENE_INT = 1, MV_GENE_OHE = 2 };

/* constraint op codes: one op == one constraint column, evaluated on the ML-space row
 * x_f (default_problem.py:93-97 then constraints.evaluate numpy path). */
enum {
  MV_OP_DIFF = 1,          /* x[a0] - x[a1]                        botnet_constraints.py:283-285 */
  MV_OP_RATIO_SAFE = 2,    /* (x[a1]!=0 ? x[a0]/x[a1] : 0) - k0     botnet_constraints.py:304-306 */
  MV_OP_ABS_SUMDIFF = 3,   /* |sum(pool[a0:a1]) - sum(pool[a1:a2])| botnet_constraints.py:127-148 */
  MV_OP_LCLD_INSTALL = 4,  /* |x3 - x0 r (1+r)^x1/((1+r)^x1-1)| - k0, r=x2/1200  lcld:174-177 */
  MV_OP_LCLD_TERM = 5,     /* |(36-x[a0])(60-x[a0])|               lcld_constraints.py:186 */
  MV_OP_ABS_RATIO = 6,     /* |x[a0] - x[a1]/x[a2]|                lcld_constraints.py:189-207 */
  MV_OP_MONTHDIFF = 7,     /* |x[a0] - (month(x[a1]) - month(x[a2]))| lcld_constraints.py:195-201 */
  MV_OP_RATIO_MASKED = 8,  /* |x[a0] - (x[a2]==0|inf|nan ? -1 : x[a1]/x[a2])| lcld:210-216 */
  MV_OP_XOR_AUG = 9,       /* |x[a0] - xor(x[a1]>=k0, x[a2]>=k1)|  examples/utils.py:7-29 */
  /* tensor-path ops (constraints.evaluate(use_tensors=True), the C-PGD loss; fp32, run by
   * mv_pgd_* only).  Tensor programs also use DIFF, ABS_SUMDIFF, ABS_RATIO and MONTHDIFF. */
  MV_OP_TF_INSTALL_MIN = 10,      /* min(|x[a3]-inst(36)|, |x[a3]-inst(60)|) - k0, inst(t) =
                                     x[a0] r (1+r)^t/((1+r)^t-1), r = x[a2]/1200  lcld:87-105 */
  MV_OP_TF_HINGE_DIFF = 11,       /* max(k0 + x[a0] - x[a1], 0)            lcld:109-113 */
  MV_OP_TF_TERM_MIN = 12,         /* min(|36-x[a0]|, |60-x[a0]|)           lcld:116 */
  MV_OP_TF_RATIO_ALPHA_NEG = 13,  /* |x[a0] - (isnan(x[a1]/x[a2]) ? -1 : x[a1]/(x[a2]+k0))|  lcld:147-151 */
  MV_OP_TF_RATIO_ALPHA_ZERO = 14, /* isnan(x[a0]-x[a1]) ? 0 : x[a0]/(x[a1]+k0)   botnet:250-269 */
  MV_OP_TF_ABS_SUMDIFF_OFF = 15,  /* |sum(pool[a0:a1]) - sum(pool[a1:a2])| - k0  botnet:55-75 */
  /* user-defined column (engine extension; no reference counterpart): a postfix expression
   * over the row, interpreted on the device in fp64 (mv_engine_*) or, as a tensor-path column
   * of mv_pgd_*, in fp32 together with its reverse-mode derivative.  op_arg = (a0 offset of its
   * first word in expr_code, a1 word count, a2 maximum stack depth, 0).  mv_engine_create and
   * mv_pgd_create simulate every such column and refuse a malformed one (MV_ERR_ARG), so the
   * device only ever interprets checked code. */
  MV_OP_EXPR = 16,
};

/* MV_OP_EXPR bytecode: int32 words, postfix, operands inline; a binary operator pops b, then
 * a, and pushes a . b (the left operand was pushed first).  Semantics are numpy's on fp64. */
enum {
  MV_X_FEAT = 1,   /* X f      push x[f]                         0 <= f < D */
  MV_X_CONST = 2,  /* K i      push expr_const[i]                0 <= i < n_expr_const */
  MV_X_SUMF = 3,   /* SUMF o0 o1  push 0.0 + x[idx_pool[o0]] + ... + x[idx_pool[o1-1]], left to
                      right; 0 <= o0 <= o1 <= n_pool */
  MV_X_ADD = 4, MV_X_SUB = 5, MV_X_MUL = 6,
  MV_X_DIV = 7,    /* IEEE: x/0 = +-inf or NaN */
  MV_X_MIN = 8, MV_X_MAX = 9,  /* np.minimum / np.maximum: NaN propagates */
  MV_X_MOD = 10,   /* np.mod: the result takes the divisor's sign */
  MV_X_POW = 11,   /* pow(a, b), the pow of MV_OP_LCLD_INSTALL */
  MV_X_LT = 12, MV_X_LE = 13, MV_X_GT = 14, MV_X_GE = 15, MV_X_EQ = 16, MV_X_NE = 17, /* 1.0/0.0 */
  MV_X_AND = 18, MV_X_OR = 19, MV_X_XOR = 20,  /* on the truth values a != 0, b != 0 */
  MV_X_NEG = 21, MV_X_ABS = 22, MV_X_FLOOR = 23,
  MV_X_NOT = 24,   /* a == 0 */
  MV_X_ISNAN = 25, MV_X_ISINF = 26,
  MV_X_WHERE = 27, /* pops b, a, c; pushes c != 0 ? a : b */
};
/* Limits of one MV_OP_EXPR column.  MV_EXPR_MAX_TAPE (mv_pgd_create only): instructions per
 * column; every instruction's value is kept on a tape for the reverse sweep. */
enum { MV_EXPR_MAX_DEPTH = 8, MV_EXPR_MAX_WORDS = 256, MV_EXPR_MAX_TAPE = 64 };

typedef struct mv_problem_desc {
  int32_t D;                  /* ML feature count */
  int32_t V;                  /* genetic length (n_var) */
  int32_t Dm;                 /* mutable feature count (mutable_mask.sum()) */
  int32_t C;                  /* constraint count */
  int32_t n_ohe;              /* mutable one-hot groups */
  const int32_t* gene_kind;   /* host [V] MV_GENE_* */
  const int32_t* gene_feat;   /* host [V] feature (REAL/INT) or group index (OHE) */
  const int32_t* ohe_offsets; /* host [n_ohe+1] CSR offsets into ohe_feats */
  const int32_t* ohe_feats;   /* host [..] features of each group, category order */
  const int32_t* mut_feats;   /* host [Dm] mutable features, ascending */
  const double* ml_scale;     /* host [D] ML MinMaxScaler scale_ (NULL: identity) */
  const double* ml_min;       /* host [D] ML MinMaxScaler min_   (NULL: identity) */
  const int32_t* op_code;     /* host [C] MV_OP_* */
  const int32_t* op_arg;      /* host [C*4] integer operands */
  const double* op_karg;      /* host [C*2] real operands */
  int32_t n_pool;             /* index pool size for MV_OP_ABS_SUMDIFF */
  const int32_t* idx_pool;    /* host [n_pool] */
  double tol;                 /* constraints <= tol -> 0  (1e-3 in every reference class) */
  int32_t norm;               /* 2 = L2, 0 = Linf  (default_problem.py:80-91) */
  int32_t scale_objectives;   /* f2 MinMax scaling (utils.py:11-22) */
  /* MV_OP_EXPR bytecode (appended: a zero-initialised struct describes a program without
   * EXPR columns) */
  int32_t n_expr_code;        /* code words of all EXPR columns */
  const int32_t* expr_code;   /* host [n_expr_code] */
  int32_t n_expr_const;       /* constants */
  const double* expr_const;   /* host [n_expr_const] */
} mv_problem_desc;

typedef struct mv_model_desc {
  int32_t n_layers;           /* Dense layers; hidden relu, last softmax */
  const int32_t* dims;        /* host [n_layers+1], dims[0] == D */
  const float* const* W;      /* host per layer [dims[l] x dims[l+1]] row-major (Keras kernel) */
  const float* const* b;      /* host per layer [dims[l+1]] */
} mv_model_desc;

typedef struct mv_engine mv_engine;

const char* mv_last_error(void);
int mv_device_count(int32_t* n);

/* Upload problem constants + classifier weights to `device`.  model may be NULL: a
 * constraints-only engine, or the engine behind a host classifier plugin (mv_evaluate then
 * leaves f1 to the caller; mv_attack_run needs a model). */
int mv_engine_create(int32_t device, const mv_problem_desc* problem, const mv_model_desc* model,
                     mv_engine** out);
void mv_engine_destroy(mv_engine* e);

/* Bind B initial states (host arrays, copied).  xl/xu are the per-state feature bounds
 * Constraints.get_feature_min_max(dynamic_input=x) (moeva2.py:141-142).  Derives on device:
 * encoder MinMax (feature_encoder.py:39-40), genetic bounds (:145-163), the initial
 * genetic vector (sampling.py:64-78) and the immutable-feature fold of the first layer. */
int mv_set_states(mv_engine* e, int32_t B, const double* x_init, const double* xl,
                  const double* xu, const int32_t* minimize_class, void* stream);

/* DefaultProblem._evaluate for n rows per bound state.
 * genes dev [B][n][V] -> F dev [B][n][3] (f1 misclassification, f2 distance, f3 constraint sum);
 * G dev [B][n][C] (constraint values after the tol clamp and G*(G>0)) or NULL. */
int mv_evaluate(mv_engine* e, int32_t n, const double* genes, double* F, double* G, void* stream);

/* FeatureEncoder.genetic_to_ml (feature_encoder.py:129-130) on device, for host-evaluated
 * plugins (a Constraints subclass without a device program, a non-Dense classifier):
 * genes dev [B][n][V] -> x dev [B][n][D] with the bound states' x_init. */
int mv_decode(mv_engine* e, int32_t n, const double* genes, double* x, void* stream);

/* Every entry point taking device buffers fails with MV_ERR_ARG when a buffer is device
 * memory of another GPU than the engine's (mlp's, objcalc's; for mv_survive and
 * mv_select_parents, which take no engine: the current device's). */
/* Constraints.evaluate (numpy path: values <= tol set to 0) on ML-space rows:
 * x dev [n][D] -> G dev [n][C].  Works on an engine created without a model. */
int mv_constraints(mv_engine* e, int32_t n, const double* x, double* G, void* stream);

/* R-NSGA-III AspirationPointSurvival._do + NonDominatedSorting + niching, batched over B
 * independent populations of N merged individuals (pymoo 0.4.2.2 rnsga3.py/nsga3.py).
 * F dev [B][N][3]; ref_points dev [R][3]; state in/out dev: ideal [B][3], worst [B][3],
 * extreme [B][3][3], has_extreme [B] (0 before the first call).
 * Outputs dev: survivors [B][n_survive] (merged indices, new population order),
 * rank [B][N] (front index, -1 = unranked) and, for the fronts-ordered individuals
 * (order [B][N], count n_ranked [B]): niche [B][N], dist [B][N].  Any output may be NULL
 * except survivors.  Requires N <= 1024 (above 512 the dominance bitsets live in an HBM
 * scratch), R <= 640. */
int mv_survive(int32_t B, int32_t N, int32_t n_survive, const double* F, int32_t R,
               const double* ref_points, double mu, uint64_t seed, int32_t gen,
               double* ideal, double* worst, double* extreme, int32_t* has_extreme,
               int32_t* survivors, int32_t* rank, int32_t* order, int32_t* n_ranked,
               int32_t* niche, double* dist, double* nadir, void* stream);

/* mv_survive on a chosen kernel instance: wide is the value mv_attack_run picks from the
 * number of states for N <= 512 (0: 512 threads per state, mv_survive's; 1: 576; 2: 1024;
 * anything else is MV_ERR_ARG).  Above N 512 there is one instance and wide is ignored.
 * Every instance computes the same bits. */
int mv_survive_wide(int32_t B, int32_t N, int32_t n_survive, const double* F, int32_t R,
                    const double* ref_points, double mu, uint64_t seed, int32_t gen,
                    double* ideal, double* worst, double* extreme, int32_t* has_extreme,
                    int32_t* survivors, int32_t* rank, int32_t* order, int32_t* n_ranked,
                    int32_t* niche, double* dist, double* nadir, int32_t wide, void* stream);

/* TournamentSelection(comp_by_cv_then_random) for B populations of P: parents dev
 * [B][ceil(O/2)][2] (population positions). */
int mv_select_parents(int32_t B, int32_t P, int32_t O, uint64_t seed, int32_t gen,
                      int32_t* parents, void* stream);

/* MixedVariableCrossover(two-point) + MixedVariableMutation(PM, eta 20), no evaluation:
 * pop dev [B][P][V], parents dev [B][O/2][2] -> off dev [B][O][V]. */
/* Crossover of mv_variation / mv_attack_run: kind 0 = two-point (moeva2.py:90-101, the
 * reference's operator; default), 1 = SBX (SimulatedBinaryCrossover, pymoo 0.4.2.2
 * real_sbx / int_sbx semantics with distribution index eta, prob_per_variable 0.5; the
 * stale comment at moeva2.py:87 names prob 0.9, eta 30).  prob: mating-level probability. */
int mv_set_crossover(mv_engine* e, int32_t kind, double eta, double prob);
int mv_variation(mv_engine* e, int32_t P, int32_t O, uint64_t seed, int32_t gen,
                 const double* pop, const int32_t* parents, double* off, void* stream);

/* Classifier.predict_proba (classifier.py:23-29) for a Dense(relu)...Dense(softmax)
 * model: x dev [n][dims[0]] (ML-scaled, fp64, cast to fp32 like Keras) -> proba dev
 * [n][n_out] fp64. */
typedef struct mv_mlp mv_mlp;
int mv_mlp_create(int32_t device, const mv_model_desc* model, mv_mlp** out);
void mv_mlp_destroy(mv_mlp* m);
int mv_mlp_predict(mv_mlp* m, int32_t n, const double* x, double* proba, void* stream);

/* ObjectiveCalculator._calculate_objective (objective_calculator.py:44-84) batched over B
 * initial states x n candidates (ML space), the scoring behind success_rate_3d (:106-119)
 * and get_successful_attacks (:152-223).  Per row: CV = calc_constraint_violation of
 * [constraints.evaluate(x) | get_one_hot_encoding_constraints(type_mask, x)] (utils.py:43-54),
 * f1 = predict_proba(ml_scaler(x))[:, minimize_class], f2 = ||mm(x_init) - mm(x)||_{2|inf}
 * on the min_max_scaler.  The constraint program is taken from a (model-less) engine, the
 * classifier from an mv_mlp. */
typedef struct mv_objcalc_desc {
  int32_t D;                  /* ML feature count */
  int32_t n_ohe;              /* one-hot groups of the FULL type mask, get_ohe_masks order */
  const int32_t* ohe_offsets; /* host [n_ohe+1] CSR offsets */
  const int32_t* ohe_feats;   /* host [..] features of each group */
  const double* mm_scale;     /* host [D] min_max_scaler scale_ (distance) */
  const double* mm_min;       /* host [D] min_max_scaler min_ */
  const double* ml_scale;     /* host [D] ml_scaler scale_, or NULL (ml_scaler None) */
  const double* ml_min;       /* host [D] or NULL */
  int32_t norm;               /* 2 = L2, 0 = Linf */
} mv_objcalc_desc;
typedef struct mv_objcalc mv_objcalc;
int mv_objcalc_create(int32_t device, const mv_objcalc_desc* desc, mv_objcalc** out);
void mv_objcalc_destroy(mv_objcalc* o);
/* x_init dev [B][D], x dev [B][n][D] -> obj dev [B][n][3] (CV, f1, f2) and range_bad dev
 * [B][n] (1 where the scaled row or origin leaves [-1e-4, 1+1e-4]: the reference asserts,
 * objective_calculator.py:72-76). */
int mv_objcalc_run(mv_objcalc* o, mv_engine* constraints, mv_mlp* classifier, int32_t B,
                   int32_t n, const double* x_init, const double* x, int32_t minimize_class,
                   double* obj, int32_t* range_bad, void* stream);
/* The same scoring with the constraint matrix and / or the class probabilities supplied by
 * the caller (device buffers): G dev [B*n][C] (Constraints.evaluate(x_f), C >= 0) and proba
 * dev [B*n][n_out].  This is the plugin path of ObjectiveCalculator._calculate_objective
 * (objective_calculator.py:44-84) for a Constraints subclass without a device program or a
 * predict_proba model that is not a Dense MLP: the host evaluates the plugin, the device
 * does the one-hot term, the CV sum, the ML/min-max scaling checks and the distance. */
int mv_objcalc_score(mv_objcalc* o, int32_t B, int32_t n, const double* x_init, const double* x,
                     const double* G, int32_t C, const double* proba, int32_t n_out,
                     int32_t minimize_class, double* obj, int32_t* range_bad, void* stream);
/* ---- Tree-ensemble classifiers (engine extension; the reference takes any predict_proba
 * model, classifier.py:11-29): scikit-learn's RandomForestClassifier / ExtraTreesClassifier /
 * DecisionTreeClassifier predict_proba, restated in moeva2_amd/models/forest.py.  A row is
 * cast to fp32 (as sklearn casts X); at an inner node it goes left when (double)x[feature] <=
 * threshold, else right (so a NaN goes right); the probability is the fp64 sum of the trees'
 * leaf rows in tree order, starting from 0.0, divided by n_trees.
 * Tables (host arrays): the nodes of tree t are tree_root[t] .. tree_root[t+1]-1, root first.
 * A node with feature < 0 is a leaf whose row is leaf_value[-feature - 1].
 * Refused with MV_ERR_ARG: n_classes outside 2..8, n_trees < 1, n_nodes above INT32_MAX, a
 * split feature outside [0, n_features), a leaf index outside leaf_value, a child index that
 * is not greater than its parent's or lies outside its own tree (so no walk can cycle), a
 * node with two parents.  The device only walks checked tables. */
typedef struct mv_forest_desc {
  int32_t n_features;         /* D: the width of a row */
  int32_t n_classes;          /* 2..8 */
  int32_t n_trees;
  int32_t n_leaves;
  int64_t n_nodes;
  const int32_t* feature;     /* host [n_nodes] split feature, or -(leaf index) - 1 */
  const double* threshold;    /* host [n_nodes] */
  const int32_t* left;        /* host [n_nodes] (unused at a leaf) */
  const int32_t* right;       /* host [n_nodes] */
  const int32_t* tree_root;   /* host [n_trees], ascending from 0 */
  const double* leaf_value;   /* host [n_leaves][n_classes]: value / normalizer, fp64 */
} mv_forest_desc;
typedef struct mv_forest mv_forest;
/* Classifier.predict_proba for a forest (the mv_mlp_* analogue): x dev [n][n_features]
 * (ML-scaled, fp64) -> proba dev [n][n_classes] fp64, the restatement's bits. */
int mv_forest_create(int32_t device, const mv_forest_desc* forest, mv_forest** out);
void mv_forest_destroy(mv_forest* f);
int mv_forest_predict(mv_forest* f, int32_t n, const double* x, double* proba, void* stream);
/* Make a forest the engine's classifier: mv_evaluate, mv_attack_run and the history then take
 * f1 = proba[minimize_class] from k_forest where they take it from an MLP kernel otherwise
 * (mv_get_mlp_kernel reports 8).  Only on an engine created with model == NULL, once, and
 * before mv_set_states (MV_ERR_STATE otherwise; no device call is made then);
 * forest->n_features must be the problem's D.  The engine keeps the full gene layout. */
int mv_engine_set_forest(mv_engine* e, const mv_forest_desc* forest);
/* mv_objcalc_run with a forest as the classifier. */
int mv_objcalc_run_forest(mv_objcalc* o, mv_engine* constraints, mv_forest* classifier,
                          int32_t B, int32_t n, const double* x_init, const double* x,
                          int32_t minimize_class, double* obj, int32_t* range_bad, void* stream);

/* ---- Gradient-boosted tree classifiers (engine extension): scikit-learn's
 * GradientBoostingClassifier (loss "log_loss") / HistGradientBoostingClassifier predict_proba,
 * restated in moeva2_amd/models/boost.py.  The tables are mv_forest_desc's with one scalar per
 * leaf (learning rate included); trees are stage-major: tree t adds its leaf to
 * raw[t % n_outputs], raw starts at base, in tree order in fp64.  Two classes (n_outputs 1):
 * p1 = 1 / (1 + E(-raw[0])), p0 = 1 - p1.  More: e[k] = E(raw[k] - max raw),
 * p[k] = e[k] / ((e[0] + e[1]) + e[2] + ...).  E is mv_det_exp's function on host and device.
 * Refused with MV_ERR_ARG: everything mv_forest_desc's rules refuse, n_outputs other than 1
 * for two classes or n_classes for more, n_trees not a multiple of n_outputs, a base or leaf
 * value that is not finite. */
typedef struct mv_boost_desc {
  int32_t n_features;         /* D: the width of a row */
  int32_t n_classes;          /* 2..8 */
  int32_t n_outputs;          /* raw scores: 1 when n_classes == 2, else n_classes */
  int32_t n_trees;            /* stages * n_outputs */
  int32_t n_leaves;
  int64_t n_nodes;
  const int32_t* feature;     /* host [n_nodes] split feature, or -(leaf index) - 1 */
  const double* threshold;    /* host [n_nodes] */
  const int32_t* left;        /* host [n_nodes] (unused at a leaf) */
  const int32_t* right;       /* host [n_nodes] */
  const int32_t* tree_root;   /* host [n_trees], ascending from 0 */
  const double* leaf_value;   /* host [n_leaves] fp64 */
  const double* base;         /* host [n_outputs] fp64 */
} mv_boost_desc;
/* A boosted ensemble behind the forest handle: mv_forest_predict, mv_forest_destroy and
 * mv_objcalc_run_forest take it unchanged and run k_boost. */
int mv_boost_create(int32_t device, const mv_boost_desc* boost, mv_forest** out);
/* mv_engine_set_forest for a boosted ensemble: the same preconditions and error codes (an
 * engine created with model == NULL, no tree ensemble set yet, before mv_set_states:
 * MV_ERR_STATE otherwise, no device call; boost->n_features must be the problem's D).
 * mv_get_mlp_kernel then reports 9 (k_boost reading its nodes from global memory) or 10
 * (k_boost walking a per-workgroup LDS copy: the packed nodes fit 64 KiB). */
int mv_engine_set_boost(mv_engine* e, const mv_boost_desc* boost);

/* ---- Kernel machines and logistic regression (engine extension): scikit-learn's SVC / NuSVC
 * (probability=True, two classes) and LogisticRegression predict_proba, restated in
 * moeva2_amd/models/svm.py.  Per row, cast to fp32 first: s_v = the fma chain over the features
 * in ascending order of x.v (linear, poly) or (x - v)^2 (rbf), from 0; K_v = s_v (linear),
 * powi(gamma * s_v + coef0, degree) (poly, libsvm's square-and-multiply) or E(-(gamma * s_v))
 * (rbf; E is mv_det_exp's function); dec[o] = sum over v ascending of coef[o][v] * K_v (multiply,
 * then add, from 0), then + intercept[o]; without coef dec[o] = K_o + intercept[o].  Links:
 * 0 = Platt's sigmoid of -dec[0] with probA / probB, clipped to [1e-7, 1 - 1e-7], then libsvm's
 * pairwise coupling for two classes (eps 0.0025, at most 100 iterations); 1 = p1 =
 * 1 / (1 + E(-dec[0])), p0 = 1 - p1; 2 = the softmax of mv_boost_desc.
 * Refused with MV_ERR_ARG: n_vec < 1, n_features < 1, n_vec * n_features > 2^24, classes outside
 * 2..8, a kernel or link outside the lists, links 0 / 1 without (2 classes, n_out 1), link 2
 * without (3..8 classes, n_out == n_classes), no coef with n_vec != n_out, a degree outside
 * 0..64, any entry or parameter that is not finite. */
typedef struct mv_svm_desc {
  int32_t n_features;       /* D: the width of a row */
  int32_t n_classes;        /* 2..8 */
  int32_t n_out;            /* decisions: 1 for two classes, else n_classes */
  int32_t n_vec;            /* support vectors, or coefficient rows (no coef) */
  int32_t kernel;           /* 0 linear, 1 poly, 2 rbf */
  int32_t degree;           /* poly */
  int32_t link;             /* 0 platt + coupling, 1 sigmoid, 2 softmax */
  double gamma, coef0;      /* poly, rbf */
  double probA, probB;      /* link 0 */
  const double* vectors;    /* host [n_vec][n_features] */
  const double* coef;       /* host [n_out][n_vec], or NULL: identity */
  const double* intercept;  /* host [n_out] */
} mv_svm_desc;
/* Such a model behind the forest handle: mv_forest_predict, mv_forest_destroy and
 * mv_objcalc_run_forest take it unchanged and run k_svm. */
int mv_svm_create(int32_t device, const mv_svm_desc* svm, mv_forest** out);
/* mv_engine_set_boost for such a model: the same preconditions and error codes (an engine
 * created with model == NULL, no other classifier set, before mv_set_states: MV_ERR_STATE
 * otherwise, no device call; svm->n_features must be the problem's D).  mv_get_mlp_kernel then
 * reports 11 (k_svm). */
int mv_engine_set_svm(mv_engine* e, const mv_svm_desc* svm);

typedef struct mv_attack_params {
  int32_t n_gen;          /* Moeva2 n_gen (termination "n_gen") */
  int32_t pop_size;       /* P = n_ref_points + n_obj (203 for n_pop 200) */
  int32_t n_offsprings;   /* O (even) */
  uint64_t seed;          /* Moeva2 seed */
  int32_t n_ref;          /* R reference points */
  const double* ref_points; /* host [R][3] */
  double mu;              /* RNSGA3 mu (0.05) */
  int32_t history;        /* 0 none, 1 "reduced" (F), 2 "full" (F|G) */
} mv_attack_params;

/* Whole attack on device: init population + evaluate + (n_gen-1) x {select, vary+evaluate,
 * survive}, no host round trip.  Asynchronous on `stream`.  Replaces Moeva2.generate's
 * per-state pymoo.minimize calls (moeva2.py:128-171, 194-205) for ALL bound states.
 * Schedule: per generation the row kernel (k_genc for wide IDENT rows such as botnet,
 * k_narrow for LCLD-shaped rows, else k_gen + k_cons; a program with MV_OP_EXPR columns
 * always k_gen + k_consx), the classifier (k_mlp2 / k_mlpw /
 * k_mlp) and k_survive (survival + the next tournament), the states split into up to 4
 * groups, each chain on its own stream. */
int mv_attack_run(mv_engine* e, const mv_attack_params* params, void* stream);
/* 0: auto (default), 1: per-phase kernel chain -- the same schedule.  2 (the retired
 * whole-attack kernel, measured slower than the chain) is rejected with MV_ERR_ARG. */
int mv_set_attack_mode(mv_engine* e, int32_t mode);
/* Random streams of the bound states (no reference counterpart; an engine option).
 * enabled = 0 (default, the reference's behaviour): every state draws from the same Philox
 * stream, as Moeva2 re-seeds each state's pymoo.minimize with the same seed
 * (moeva2.py:158-165).  enabled = 1: state b draws from its own stream, keyed by its GLOBAL
 * index first_state + b (pass the shard's offset under sharding, so results do not depend on
 * the GPU count).  Each state's attack is statistically the same either way; across states
 * the outcomes become independent, which is what the end-to-end parity test needs to resolve
 * 1 pp (tests/test_gpu_e2e.py).  Applies to mv_attack_run and mv_variation. */
int mv_set_state_streams(mv_engine* e, int32_t enabled, int64_t first_state);
/* Classifier precision of the engine's fitness path (mv_evaluate, mv_attack_run): 0 = fp32
 * (default; the parity mode: exact fp32 products on v_mfma_f32_16x16x4f32, as Keras computes
 * classifier.py:23-29), 1 = bf16 perf mode (hidden-layer weights and activations rounded to
 * bf16, fp32 accumulation on v_mfma_f32_16x16x32_bf16; f1 is no longer Keras's value, so
 * results are not parity results).  No reference counterpart: an engine option. */
int mv_set_mlp_precision(mv_engine* e, int32_t bf16);
/* Kept for ABI stability: the whole-attack kernel was retired, so *ms = 0 and *whole = 0. */
int mv_get_attack_time(mv_engine* e, double* ms, int32_t* whole);
/* Final population: genes dev [B][P][V], F dev [B][P][3] (either may be NULL). */
int mv_attack_population(mv_engine* e, double* genes, double* F, void* stream);
/* The final population's non-dominated members: the per-state result's X / F (moeva2.py:
 * 167-171 returns pymoo's Result, whose X / F are the last population's first front).  The
 * relation is pareto_operation.py:35-51's: i dominates j when F_i < F_j in some objective and
 * F_i > F_j in none; a member is in the front when no member of its state's final population
 * dominates it (the comparisons of a numpy any(<) / any(>) broadcast, so the mask is
 * bit-identical to one computed on the host from mv_attack_population's F).  Outputs dev:
 * front [B][P] uint8 (1 = member), offsets [B+1] int32 (state b's members are rows
 * offsets[b] .. offsets[b+1]-1, population order), X [B*P][V] / Fx [B*P][3] (worst-case size;
 * the first offsets[B] rows are written).  Any output may be NULL. */
int mv_attack_front(mv_engine* e, uint8_t* front, int32_t* offsets, double* X, double* Fx,
                    void* stream);
/* mv_attack_front's kernels on a caller's populations (no engine, as mv_survive): F dev
 * [B][P][3] and, for X, genes dev [B][P][V]; outputs as mv_attack_front's, front and offsets
 * required, X / Fx may be NULL.  P <= 1022.  Synchronises the stream before it returns. */
int mv_front(int32_t B, int32_t P, int32_t V, const double* F, const double* genes,
             uint8_t* front, int32_t* offsets, double* X, double* Fx, void* stream);
/* History rows per state = P + (n_gen-1)*O, width 3 (reduced) or 3+C (full): hist [B][rows][w]
 * a device buffer or page-locked host memory (hipHostMalloc / registered: one DMA). */
int mv_attack_history(mv_engine* e, double* hist, void* stream);
/* What the last mv_attack_run's survival calls took over from the call before them (engine
 * extension; results do not depend on it).  A state's survivors keep their objectives, so
 * when all of them came from front 0 the next call skips the dominance work among them, and
 * when the ideal point and the nadir keep their bits the next call takes the survivors'
 * niche and distance from their pool slots instead of sweeping the reference directions.
 * Host arrays [B]: dom_skipped the calls that skipped dominance work items (the population
 * holds a whole 64-row block), assoc_reused the calls that reused the association.  Both
 * are zero before the first attack on the bound states, and stay zero with MV_SURV_CARRY=0
 * in the environment when the engine was created; mv_survive (no engine) carries nothing.
 * Synchronises the device. */
int mv_get_survival_carry(mv_engine* e, int32_t* dom_skipped, int32_t* assoc_reused);
/* The attack's gene layout for the bound states (engine extension; no reference
 * counterpart).  mv_set_states finds the genes no attack on those states can change --
 * integer genes whose bounds are equal and whose initial value is that bound in every state
 * (crossover swaps equal values, mutation clamps back to the bound; botnet: 120 of 432) --
 * and the attack neither stores, moves nor sums them: their features are evaluated as
 * immutable features (decoded from x_init, folded into the layer-1 bias, absent from f2's
 * sum).  Every draw stays defined over all V genes, so the populations are those of the
 * full layout; f1 / f2 follow the engine's summation order over the stored genes
 * (oracle/device_order.py, `fixed`).  mv_evaluate / mv_decode / mv_variation always use
 * every gene.  stored (may be NULL) [V] receives 1 for a stored gene, 0 for a fixed one;
 * *n_stored the stored count (= V when nothing is fixed, or MV_COMPACT=0). */
int mv_get_stored_genes(mv_engine* e, int32_t* stored, int32_t* n_stored);
/* The layout mv_set_states would derive for B states (host arrays as mv_set_states; host
 * computation only, no device work): stored [V] 1 / 0 and *n_stored, as mv_get_stored_genes
 * reports after binding them. */
int mv_gene_layout(mv_engine* e, int32_t B, const double* x_init, const double* xl,
                   const double* xu, int32_t* stored, int32_t* n_stored);
/* Fix the layout of the NEXT mv_set_states call (one call only; the request is consumed by
 * it, refused or not, so a later binding on a shared engine derives its own): stored [V]
 * (1 = stored) as
 * mv_gene_layout returned it for the WHOLE job, so a job split into batches or shards
 * (Moeva2.generate_sharded) runs every state in the same layout -- a state's f1 / f2
 * summation order, hence its trajectory, then does not depend on which states share its
 * batch.  mv_set_states fails with MV_ERR_ARG when an unstored gene is not fixed in a bound
 * state.  stored = NULL returns to deriving the layout from each bound batch (default). */
int mv_set_gene_layout(mv_engine* e, const int32_t* stored, int32_t V);
/* Per-kernel timing of the last mv_attack_run when enabled (one state group then): each
 * profiled launch -- the row kernel(s), the classifier and k_survive of every generation --
 * is made with hipExtLaunchKernelGGL and a start / stop HIP event pair, which stamp the
 * kernel's own execution (no dispatch gap); summed ms.  A step that launches no kernel
 * (k_cons under k_genc / k_narrow) reads 0. */
int mv_set_profiling(mv_engine* e, int32_t enabled);
int mv_get_kernel_times(mv_engine* e, double* vary_ms, double* mlp_ms, double* survive_ms,
                        int32_t* n_generations);
/* Same events, split by kernel: ms[0] the row kernel's variation part (k_gen; k_genc or
 * k_narrow: the whole row kernel), ms[1] k_cons (constraints + f3; 0 when k_genc or k_narrow
 * ran), ms[2] the classifier (f1), ms[3] k_survive (survival + next tournament), summed over
 * the profiled generations. */
int mv_get_phase_times(mv_engine* e, double* ms, int32_t* n_generations);
/* The kernels an attack generation runs for its offspring rows under the engine's current
 * options: 0 = k_gen then k_cons, 1 = k_narrow (one lane per row, both in one launch; the
 * k_cons events then bracket nothing), 2 = k_genc (k_gen and k_cons as two phases of one
 * launch; likewise).  Lets a profiler attribute ms[0] + ms[1] of mv_get_phase_times. */
int mv_get_row_kernel(mv_engine* e, int32_t* kind);
/* The classifier kernel an attack generation runs: 0 = k_mlp (one tile of rows per
 * workgroup, any widths), 1 = k_mlp2 reading the child genes (no fp32 ML row is written),
 * 2 = k_mlp2 reading the fp32 ML rows, 4 = k_mlpw (bf16 weights), 5 = k_mlpw32 (fp32 wide
 * nets: 64-row tiles, one activation buffer), 6 / 7 = k_mlpr reading the genes / the fp32 ML
 * rows, 8 = k_forest (a tree ensemble, mv_engine_set_forest), 9 / 10 = k_boost (a boosted
 * ensemble, mv_engine_set_boost) over global memory / LDS, 11 = k_svm (a kernel machine or
 * logistic regression, mv_engine_set_svm), -1 = no device classifier
 * (3, the retired k_mlp2x, is no longer returned).
 * Lets a profiler price the ML-row bytes of the row kernel and the classifier. */
int mv_get_mlp_kernel(mv_engine* e, int32_t* kind);

/* Device index checks (debug builds compiled with -DMV_CHECKS, `make checks`): synchronises
 * the device, then returns and clears the first failed check of the row, classifier and
 * survival kernels since the last call -- record[0] check code (csrc/check.h; 0 = none),
 * [1] workgroup, [2] thread, [3] value, [4] bound, [5] number of failures -- and *compiled = 1
 * in a checks build (0 otherwise: record is all zero).  A checks build also fails
 * mv_attack_population with MV_ERR_STATE when a check failed.  No reference counterpart. */
int mv_debug_checks(int32_t* record, int32_t* compiled);
/* Checks builds: the inputs of the first survival whose survivors were not distinct (check
 * 26) -- out[3096] doubles: [0] 1 if valid, [1] generation, [2] state in its group, [3] N,
 * [4..6] carried ideal, [7..9] worst, [10..18] extremes, [19] has_extreme, [20] n_survive,
 * [21] seed (uint64 bits), [24..24+3N) merged F.  Cleared by the call; zeros otherwise. */
int mv_debug_survival_dump(double* out);

/* The engine's pow for the variation operators (host build of csrc/detmath.h det_pow, the
 * same IEEE operation sequence as the device code): out[i] = det_pow(x[i], y[i]) for host
 * arrays.  Replaces np.power in softmax_mutation.py:77-103 (polynomial mutation) and the
 * SBX option's calc_betaq; oracle/device_order.py:det_pow restates it. */
int mv_det_pow(int64_t n, const double* x, const double* y, double* out);
/* The engine's exp for the boosted ensembles' sigmoid and softmax (host build of csrc/detmath.h
 * det_exp2(x, 0.0): fdlibm's exp, the same IEEE operation sequence as k_boost's):
 * out[i] = E(x[i]) for host arrays.  models/boost.py's specification calls it. */
int mv_det_exp(int64_t n, const double* x, double* out);
/* The feature sums of k_svm (host build of csrc/svm.h svm_term, one fma per feature in
 * ascending order from 0): out[i][v] = sum_j x[i][j] * vectors[v][j], or of
 * (x[i][j] - vectors[v][j])^2 when rbf != 0, for host arrays x [n][D], vectors [n_vec][D].
 * models/svm.py's specification calls it. */
int mv_svm_sums(int64_t n, int32_t D, int32_t n_vec, int32_t rbf, const double* x,
                const double* vectors, double* out);

/* ---- C-PGD: the constrained gradient attack (src/attacks/pgd/atk.py:74-163 on ART's PGD
 * loop, src/attacks/pgd/classifier.py:107-332 loss_gradient), whole loop on device.  All
 * device buffers are fp32; rows are ML-scaled (scaler.transform(x)) unless stated.
 * An MV_OP_EXPR column is evaluated in fp32 on XF(f) = (x[f] - min[f]) / scale[f] with the value
 * semantics of the MV_X_* table (POW is powf) and differentiated by a reverse sweep with
 * autograd's rules; the comparisons, AND OR XOR NOT ISNAN ISINF and the
 * condition of WHERE pass no gradient to their operands. */
typedef struct mv_pgd_desc {
  int32_t D;                  /* ML feature count (== model dims[0]) */
  const double* ml_scale;     /* host [D] ML MinMaxScaler scale_ (cast to fp32) */
  const double* ml_min;       /* host [D] min_ */
  const int32_t* mutable_mask;/* host [D] 1 = mutable */
  int32_t C;                  /* tensor program: constraint columns */
  const int32_t* op_code;     /* host [C] MV_OP_* (tensor-path subset, MV_OP_EXPR included) */
  const int32_t* op_arg;      /* host [C*4] */
  const double* op_karg;      /* host [C*2] */
  int32_t n_pool;
  const int32_t* idx_pool;    /* host [n_pool] */
  int32_t n_ohe;              /* repair: one-hot groups of the full type mask (0: none) */
  const int32_t* ohe_offsets; /* host [n_ohe+1] */
  const int32_t* ohe_feats;
  int32_t repair_install[4];  /* repair: amount, term, rate, installment features of the LCLD
                                 formula; repair_install[0] < 0: no formula repair */
  double tol;                 /* 1e-3 */
  /* MV_OP_EXPR bytecode, as in mv_problem_desc (appended: a zero-initialised tail describes a
   * program without EXPR columns).  Constants are rounded to fp32 once at create time. */
  int32_t n_expr_code;
  const int32_t* expr_code;   /* host [n_expr_code] */
  int32_t n_expr_const;
  const double* expr_const;   /* host [n_expr_const] */
} mv_pgd_desc;

/* loss_flags: which terms the gradient is taken of. */
enum { MV_PGD_LOSS_FLIP = 1, MV_PGD_LOSS_CONSTRAINTS = 2 };

typedef struct mv_pgd_params {
  int32_t max_iter;
  int32_t norm;        /* 2 = L2, 0 = Linf */
  double eps;
  double eps_step;
  int32_t loss_flags;  /* MV_PGD_LOSS_* */
  int32_t adaptive;    /* eta = eps 10^-(i / (max_iter / 7) + 1); needs max_iter >= 7 */
  int32_t repair;      /* x = scale(fix_features_types(unscale(x))) after every projection */
} mv_pgd_params;

typedef struct mv_pgd mv_pgd;
int mv_pgd_create(int32_t device, const mv_pgd_desc* desc, const mv_model_desc* model,
                  mv_pgd** out);
void mv_pgd_destroy(mv_pgd* p);
/* One loss_gradient: x_scaled dev [n][D], y dev [n] int32 class indices -> grad dev [n][D]
 * (raw: before mask and normalisation; may be NULL), losses dev [n][2 + C] = (cross-entropy
 * of the logits, sum of the columns, the C tensor-path columns; may be NULL).  iter is the
 * attack iteration (the "sum" constraint reduction does not depend on it). */
int mv_pgd_grad(mv_pgd* p, int32_t n, const float* x_scaled, const int32_t* y,
                int32_t loss_flags, int32_t iter, float* grad, float* losses, void* stream);
/* The attack: x_init_scaled dev [n][D] -> x_adv dev [n][D] (the last iterate), one launch.
 * y dev [n] or NULL (labels = argmax of the model's prediction on x_init_scaled). */
int mv_pgd_run(mv_pgd* p, const mv_pgd_params* params, int32_t n, const float* x_init_scaled,
               const int32_t* y, float* x_adv, void* stream);
/* Constraints.fix_features_types on feature-space (unscaled) rows, in place: dev [n][D]. */
int mv_pgd_repair(mv_pgd* p, int32_t n, float* x_feature_space, void* stream);

/* ---- Training the Dense MLP (adversarial retraining: train_model of the reference's
 * src/experiments/lcld/model.py:9-42, Keras Adam on the mean sparse cross-entropy), fp32.
 * Parameter layout of every flat [n_params] array (gradient, Adam m and v): per layer, W
 * row-major (in, out) followed by b.  A step is two launches (the batch's per-workgroup
 * gradients, then their fixed-order sum and the update); no atomics, so a result depends
 * on its inputs alone. */
typedef struct mv_train_opt {
  double lr;       /* Adam, Keras form: w -= lr_t m / (sqrt(v) + epsilon), */
  double beta1;    /* lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t)          */
  double beta2;
  double epsilon;
} mv_train_opt;

typedef struct mv_train mv_train;
/* The model limits are mv_pgd_create's (2..6 layers, hidden widths multiples of 16 up to 512,
 * 1..8 outputs, one tile's activations within LDS).  The initial weights are copied from
 * `model`; m, v and the step count start at 0. */
int mv_train_create(int32_t device, const mv_model_desc* model, const mv_train_opt* opt,
                    mv_train** out);
void mv_train_destroy(mv_train* t);
/* n_steps consecutive optimiser steps.  x_scaled dev [n][D], y dev [n] int32 class indices,
 * perm dev [n] int32 or NULL (identity).  Step s takes the rows at positions first_row +
 * s * batch ... of the permuted order, at most batch of them and none past n (a short last
 * batch divides by its own size); every step must hold a row.  step_losses dev [n_steps]
 * (each step's mean cross-entropy, before its update) or NULL. */
int mv_train_steps(mv_train* t, int32_t n, const float* x_scaled, const int32_t* y,
                   const int32_t* perm, int32_t first_row, int32_t batch, int32_t n_steps,
                   float* step_losses, void* stream);
/* Forward only over n rows: loss_and_correct dev [2] = (mean cross-entropy, rows whose
 * argmax -- the first maximum -- equals y, as a float: exact up to 2^24 rows). */
int mv_train_eval(mv_train* t, int32_t n, const float* x_scaled, const int32_t* y,
                  float* loss_and_correct, void* stream);
/* The reduced gradient of the mean cross-entropy over all n rows (one batch), no update:
 * grad dev [n_params], loss dev [1] (may be NULL). */
int mv_train_grad(mv_train* t, int32_t n, const float* x_scaled, const int32_t* y,
                  const int32_t* perm, float* grad, float* loss, void* stream);
/* Copies to host arrays (synchronise the stream of the last call first): W[l] [dims[l] x
 * dims[l+1]], b[l] [dims[l+1]]; m, v [n_params] (either may be NULL) and the step count. */
int mv_train_get(mv_train* t, float* const* W, float* const* b);
int mv_train_get_state(mv_train* t, float* m, float* v, int64_t* step);
/* Replace m, v (host [n_params]) and the step count: resuming, and the tests' way to a late
 * step. */
int mv_train_set_state(mv_train* t, const float* m, const float* v, int64_t step);
/* Profiling (tools/train_speed.py): with on != 0, mv_train_steps brackets each of its two
 * launches with HIP events and waits for every step; the call clears the sums, which
 * mv_train_get_kernel_times returns: device ms in k_train_grad and k_train_adam over `steps`
 * optimiser steps. */
int mv_train_set_profiling(mv_train* t, int32_t on);
int mv_train_get_kernel_times(mv_train* t, double* grad_ms, double* adam_ms, int64_t* steps);

#ifdef __cplusplus
}
#endif
#endif /* MOEVA_MI355X_H */
