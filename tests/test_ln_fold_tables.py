"""The shape tables of tests/test_gpu_ln_fold.py name, per case, the kernel that launch_gemm's rules give it; this checks the tables against
the test's restatement of those rules without a GPU (what was really launched is in profiles/ln_fold_conditioning.txt, from a kernel trace
of that file)."""
from tests.test_gpu_ln_fold import PRODUCER_CASES, SEAM_GROUPS, gemm_kernel


def test_the_case_tables_name_the_kernel_the_launch_rules_pick():
    for R, N, K, policy, kernel in PRODUCER_CASES:
        assert gemm_kernel(R, N, K, policy) == kernel, (R, N, K, policy)
    for kernel in ("k_gemm32/SK1", "k_gemm32/SK2", "k_gemm32/SK4", "k_gemm64", "k_gemm64x", "k_gemm128x"):
        assert sum(c[4] == kernel for c in PRODUCER_CASES) >= 3, kernel
    for family in ("k_gemm32", "k_gemm64", "k_gemm64x", "k_gemm128x"):       # each with a width that is no multiple of 32
        assert any(c[4].split("/")[0] == family and c[1] % 32 for c in PRODUCER_CASES), family
    for C, R, N, gelu, policy, kernel in SEAM_GROUPS:
        assert gemm_kernel(R, N, C, policy).split("/")[0] == kernel, (C, R, N, policy)
    assert {g[5] for g in SEAM_GROUPS} == {"k_gemm32", "k_gemm64", "k_gemm64x", "k_gemm128x"}
