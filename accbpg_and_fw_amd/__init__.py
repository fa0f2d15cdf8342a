"""accbpg_and_fw_amd -- MI355X-native implementation of the D-optimal-design hot path of
accbpg (DredderGun/accbpg_and_fw): BPG / ABPG / ABPG_gain with the Burg-entropy simplex
kernel, and D_opt_FW / D_opt_FW_away, behind the reference's own names and signatures.

    import accbpg_and_fw_amd as accbpg
    f, h, L, x0 = accbpg.D_opt_design(80, 200)
    x, F, G, T = accbpg.BPG(f, h, L, x0, maxitrs=1000)

All arithmetic runs in hand-written gfx950 HIP kernels (accbpg_and_fw_amd/csrc) through a
ctypes C-ABI (include/accbpg_hip.h); there is no CPU fallback.
"""
from .functions import (RSmoothFunction, DOptimalObj, PoissonRegression, KLdivRegression, LegendreFunction,
                        BurgEntropy, BurgEntropyL1, BurgEntropyL2, BurgEntropySimplex, ShannonEntropy,
                        ShannonEntropyL1, ShannonEntropySimplex, FrobeniusSymLoss, SumOf2nd4thPowers,
                        SumOf2nd4thPowersPositiveOrthant, SquaredL2Norm, SVM_fun, PolyDiv, LogisticRegression,
                        L2L1Linf)
from .algorithms import BPG, ABPG, ABPG_gain, ABPG_expo, ABDA, AIBM, AdaptFGM, UniversalGM, solve_theta
from .algorithms_fw import (FW_alg_div_step, FW_alg_descent_step, FW_alg_L0_L1_shortest_step,
                            FW_alg_L0_L1_shortest_step_steps, FW_l0l1_log_and_linear_step,
                            FW_l0l1_log_and_linear_step_steps, FW_l0l1_log_only, FW_l0l1_log_only_steps)
from .functions_lmo import lmo_simplex, lmo_l2_ball, lmo_linf_ball, lmo_l2_ball_positive_orthant, fw_direction
from .D_opt_alg import (D_opt_FW, D_opt_FW_away, D_opt_FW_batch, D_opt_FW_away_batch, D_opt_FW_device,
                        D_opt_FW_away_device, D_opt_FW_batch_device, D_opt_FW_away_batch_device,
                        D_opt_FW_div_step, D_opt_FW_descent_step, D_opt_FW_div_step_batch,
                        D_opt_FW_descent_step_batch, D_opt_FW_div_step_device, D_opt_FW_descent_step_device,
                        D_opt_FW_div_step_batch_device, D_opt_FW_descent_step_batch_device)
from .applications import (D_opt_design, D_opt_libsvm, D_opt_KYinit, D_opt_KYinit_device, D_opt_KYinit_batch,
                           Poisson_regrL1, Poisson_regrL2, KL_nonneg_regr, FrobeniusSymLossExL2Ball,
                           FrobeniusSymLossExLInfBall, FrobeniusSymLossResMeasEx, Poisson_regr_simplex,
                           Poisson_regr_simplex_acc, svm_digits_ds_divs_ball, Logistic_regr_L2L1Linf, toeplitz_matrix,
                           hard_FW_log_reg_jax, L0L1_FW_log_reg, load_a9a_data, L0L1_FW_log_reg_a9a)
from .utils import (load_libsvm_file, random_point_on_simplex, edge_point_on_simplex, get_random_float,
                    get_random_vector, random_point_in_l2_ball, generate_dataset_for_svm)
from .batched import (DOptimalBatch, BPG_batch, ABPG_batch, ABPG_gain_batch, ABPG_expo_batch, ABPG_expo_batch_steps,
                      ABDA_batch, ABDA_batch_steps, solve_batch, solve_instances)

__all__ = ["RSmoothFunction", "DOptimalObj", "PoissonRegression", "LegendreFunction", "BurgEntropy",
           "BurgEntropyL1", "BurgEntropyL2", "BurgEntropySimplex", "Poisson_regrL1", "Poisson_regrL2",
           "KLdivRegression", "ShannonEntropy", "ShannonEntropyL1", "ShannonEntropySimplex", "KL_nonneg_regr",
           "BPG", "ABPG", "ABPG_gain", "ABPG_expo", "ABDA", "solve_theta", "FW_alg_div_step", "lmo_simplex",
           "D_opt_FW", "D_opt_FW_away", "D_opt_design", "D_opt_libsvm", "D_opt_KYinit", "load_libsvm_file",
           "FrobeniusSymLoss", "SumOf2nd4thPowers", "SumOf2nd4thPowersPositiveOrthant", "SquaredL2Norm",
           "FW_alg_descent_step", "lmo_l2_ball", "lmo_linf_ball", "FrobeniusSymLossExL2Ball",
           "FrobeniusSymLossExLInfBall", "FrobeniusSymLossResMeasEx", "AIBM", "AdaptFGM", "UniversalGM",
           "Poisson_regr_simplex", "Poisson_regr_simplex_acc", "lmo_l2_ball_positive_orthant",
           "random_point_on_simplex", "edge_point_on_simplex", "get_random_float", "get_random_vector",
           "D_opt_FW_batch", "D_opt_FW_away_batch", "D_opt_FW_device", "D_opt_FW_away_device",
           "D_opt_FW_batch_device", "D_opt_FW_away_batch_device", "D_opt_KYinit_device",
           "D_opt_KYinit_batch", "D_opt_FW_div_step", "D_opt_FW_descent_step", "D_opt_FW_div_step_batch",
           "D_opt_FW_descent_step_batch", "D_opt_FW_div_step_device", "D_opt_FW_descent_step_device",
           "D_opt_FW_div_step_batch_device", "D_opt_FW_descent_step_batch_device", "SVM_fun",
           "PolyDiv", "svm_digits_ds_divs_ball", "random_point_in_l2_ball", "generate_dataset_for_svm",
           "ABPG_expo_batch", "ABPG_expo_batch_steps", "ABDA_batch", "ABDA_batch_steps",
           "LogisticRegression", "L2L1Linf", "Logistic_regr_L2L1Linf", "FW_alg_L0_L1_shortest_step",
           "FW_alg_L0_L1_shortest_step_steps", "FW_l0l1_log_and_linear_step", "FW_l0l1_log_and_linear_step_steps",
           "FW_l0l1_log_only", "FW_l0l1_log_only_steps", "fw_direction", "toeplitz_matrix", "hard_FW_log_reg_jax",
           "L0L1_FW_log_reg", "load_a9a_data", "L0L1_FW_log_reg_a9a"]
__version__ = "0.1.0"
