// Test harness kernels (NOT part of the product library): tests/testkit/librfuse_testkit.so, built by csrc/build.py next to librfuse_hip.so.
//   rft_poison_lds / rft_poison_vgprs : fill the LDS of every CU / the vector register files with NaN bit patterns (neither is cleared between
//                                       kernels), so that a kernel reading what it never wrote fails every time (tests/conftest.py)
//   rft_f16_mfma_load                 : a long-running kernel that issues nothing but F16 MFMAs from 154 VGPRs per wave -- it leaves room for other
//                                       kernels' waves on every SIMD.  Beside it, packed-fp32 VALU instructions with op_sel on src1 read zero in
//                                       lanes 48..63 (DESIGN 4.7); tests/test_two_stream_gpu.py runs every kernel family of the library beside it.
//   rft_lane_reduce_probe             : one wave calls every fixed-order reduction of csrc/lane_reduce.h on per-lane inputs and stores every lane's
//                                       result (tests/test_lane_reduce_gpu.py pins which lane gets which value, and the order of the adds)
//   rft_block_reduce_probe            : 32 workgroups call the workgroup reductions of that header (wave-order sum, maximum over waves, halving tree)
#include <hip/hip_runtime.h>
#include "../../retrieval-fuse_amd/csrc/lane_reduce.h"      // f32x4 and the helpers under test
typedef _Float16 h8 __attribute__((ext_vector_type(8)));

__global__ __launch_bounds__(1024) void k_poison_lds(unsigned* sink) {
    extern __shared__ unsigned lds[];
    for (int i = threadIdx.x; i < 160 * 1024 / 4; i += 1024) lds[i] = 0x7fc0dead;
    __syncthreads();
    if (lds[(threadIdx.x * 37) % (160 * 1024 / 4)] == 12345u && sink) sink[0] = 1;      // keeps the stores alive
}

extern "C" int rft_poison_lds(void* stream) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_poison_lds), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_poison_lds, dim3(2048), dim3(1024), 160 * 1024, (hipStream_t)stream, (unsigned*)nullptr);
    return (int)hipGetLastError();
}

__global__ __launch_bounds__(64) void k_poison_vgprs() {
    asm volatile("v_mov_b32 v0, 0x7fc0dead\n\tv_mov_b32 v1, 0x7fc0dead\n\tv_mov_b32 v2, 0x7fc0dead\n\tv_mov_b32 v3, 0x7fc0dead\n\tv_mov_b32 v4, 0x7fc0dead\n\tv_mov_b32 v5, 0x7fc0dead\n\tv_mov_b32 v6, 0x7fc0dead\n\tv_mov_b32 v7, 0x7fc0dead\n\tv_mov_b32 v8, 0x7fc0dead\n\tv_mov_b32 v9, 0x7fc0dead\n\tv_mov_b32 v10, 0x7fc0dead\n\tv_mov_b32 v11, 0x7fc0dead\n\tv_mov_b32 v12, 0x7fc0dead\n\tv_mov_b32 v13, 0x7fc0dead\n\tv_mov_b32 v14, 0x7fc0dead\n\tv_mov_b32 v15, 0x7fc0dead\n\tv_mov_b32 v16, 0x7fc0dead\n\tv_mov_b32 v17, 0x7fc0dead\n\tv_mov_b32 v18, 0x7fc0dead\n\tv_mov_b32 v19, 0x7fc0dead\n\tv_mov_b32 v20, 0x7fc0dead\n\tv_mov_b32 v21, 0x7fc0dead\n\tv_mov_b32 v22, 0x7fc0dead\n\tv_mov_b32 v23, 0x7fc0dead\n\tv_mov_b32 v24, 0x7fc0dead\n\tv_mov_b32 v25, 0x7fc0dead\n\tv_mov_b32 v26, 0x7fc0dead\n\tv_mov_b32 v27, 0x7fc0dead\n\tv_mov_b32 v28, 0x7fc0dead\n\tv_mov_b32 v29, 0x7fc0dead\n\tv_mov_b32 v30, 0x7fc0dead\n\tv_mov_b32 v31, 0x7fc0dead\n\tv_mov_b32 v32, 0x7fc0dead\n\tv_mov_b32 v33, 0x7fc0dead\n\tv_mov_b32 v34, 0x7fc0dead\n\tv_mov_b32 v35, 0x7fc0dead\n\tv_mov_b32 v36, 0x7fc0dead\n\tv_mov_b32 v37, 0x7fc0dead\n\tv_mov_b32 v38, 0x7fc0dead\n\tv_mov_b32 v39, 0x7fc0dead\n\tv_mov_b32 v40, 0x7fc0dead\n\tv_mov_b32 v41, 0x7fc0dead\n\tv_mov_b32 v42, 0x7fc0dead\n\tv_mov_b32 v43, 0x7fc0dead\n\tv_mov_b32 v44, 0x7fc0dead\n\tv_mov_b32 v45, 0x7fc0dead\n\tv_mov_b32 v46, 0x7fc0dead\n\tv_mov_b32 v47, 0x7fc0dead\n\tv_mov_b32 v48, 0x7fc0dead\n\tv_mov_b32 v49, 0x7fc0dead\n\tv_mov_b32 v50, 0x7fc0dead\n\tv_mov_b32 v51, 0x7fc0dead\n\tv_mov_b32 v52, 0x7fc0dead\n\tv_mov_b32 v53, 0x7fc0dead\n\tv_mov_b32 v54, 0x7fc0dead\n\tv_mov_b32 v55, 0x7fc0dead\n\tv_mov_b32 v56, 0x7fc0dead\n\tv_mov_b32 v57, 0x7fc0dead\n\tv_mov_b32 v58, 0x7fc0dead\n\tv_mov_b32 v59, 0x7fc0dead\n\tv_mov_b32 v60, 0x7fc0dead\n\tv_mov_b32 v61, 0x7fc0dead\n\tv_mov_b32 v62, 0x7fc0dead\n\tv_mov_b32 v63, 0x7fc0dead\n\tv_mov_b32 v64, 0x7fc0dead\n\tv_mov_b32 v65, 0x7fc0dead\n\tv_mov_b32 v66, 0x7fc0dead\n\tv_mov_b32 v67, 0x7fc0dead\n\tv_mov_b32 v68, 0x7fc0dead\n\tv_mov_b32 v69, 0x7fc0dead\n\tv_mov_b32 v70, 0x7fc0dead\n\tv_mov_b32 v71, 0x7fc0dead\n\tv_mov_b32 v72, 0x7fc0dead\n\tv_mov_b32 v73, 0x7fc0dead\n\tv_mov_b32 v74, 0x7fc0dead\n\tv_mov_b32 v75, 0x7fc0dead\n\tv_mov_b32 v76, 0x7fc0dead\n\tv_mov_b32 v77, 0x7fc0dead\n\tv_mov_b32 v78, 0x7fc0dead\n\tv_mov_b32 v79, 0x7fc0dead\n\tv_mov_b32 v80, 0x7fc0dead\n\tv_mov_b32 v81, 0x7fc0dead\n\tv_mov_b32 v82, 0x7fc0dead\n\tv_mov_b32 v83, 0x7fc0dead\n\tv_mov_b32 v84, 0x7fc0dead\n\tv_mov_b32 v85, 0x7fc0dead\n\tv_mov_b32 v86, 0x7fc0dead\n\tv_mov_b32 v87, 0x7fc0dead\n\tv_mov_b32 v88, 0x7fc0dead\n\tv_mov_b32 v89, 0x7fc0dead\n\tv_mov_b32 v90, 0x7fc0dead\n\tv_mov_b32 v91, 0x7fc0dead\n\tv_mov_b32 v92, 0x7fc0dead\n\tv_mov_b32 v93, 0x7fc0dead\n\tv_mov_b32 v94, 0x7fc0dead\n\tv_mov_b32 v95, 0x7fc0dead\n\tv_mov_b32 v96, 0x7fc0dead\n\tv_mov_b32 v97, 0x7fc0dead\n\tv_mov_b32 v98, 0x7fc0dead\n\tv_mov_b32 v99, 0x7fc0dead\n\tv_mov_b32 v100, 0x7fc0dead\n\tv_mov_b32 v101, 0x7fc0dead\n\tv_mov_b32 v102, 0x7fc0dead\n\tv_mov_b32 v103, 0x7fc0dead\n\tv_mov_b32 v104, 0x7fc0dead\n\tv_mov_b32 v105, 0x7fc0dead\n\tv_mov_b32 v106, 0x7fc0dead\n\tv_mov_b32 v107, 0x7fc0dead\n\tv_mov_b32 v108, 0x7fc0dead\n\tv_mov_b32 v109, 0x7fc0dead\n\tv_mov_b32 v110, 0x7fc0dead\n\tv_mov_b32 v111, 0x7fc0dead\n\tv_mov_b32 v112, 0x7fc0dead\n\tv_mov_b32 v113, 0x7fc0dead\n\tv_mov_b32 v114, 0x7fc0dead\n\tv_mov_b32 v115, 0x7fc0dead\n\tv_mov_b32 v116, 0x7fc0dead\n\tv_mov_b32 v117, 0x7fc0dead\n\tv_mov_b32 v118, 0x7fc0dead\n\tv_mov_b32 v119, 0x7fc0dead\n\tv_mov_b32 v120, 0x7fc0dead\n\tv_mov_b32 v121, 0x7fc0dead\n\tv_mov_b32 v122, 0x7fc0dead\n\tv_mov_b32 v123, 0x7fc0dead\n\tv_mov_b32 v124, 0x7fc0dead\n\tv_mov_b32 v125, 0x7fc0dead\n\tv_mov_b32 v126, 0x7fc0dead\n\tv_mov_b32 v127, 0x7fc0dead\n\tv_mov_b32 v128, 0x7fc0dead\n\tv_mov_b32 v129, 0x7fc0dead\n\tv_mov_b32 v130, 0x7fc0dead\n\tv_mov_b32 v131, 0x7fc0dead\n\tv_mov_b32 v132, 0x7fc0dead\n\tv_mov_b32 v133, 0x7fc0dead\n\tv_mov_b32 v134, 0x7fc0dead\n\tv_mov_b32 v135, 0x7fc0dead\n\tv_mov_b32 v136, 0x7fc0dead\n\tv_mov_b32 v137, 0x7fc0dead\n\tv_mov_b32 v138, 0x7fc0dead\n\tv_mov_b32 v139, 0x7fc0dead\n\tv_mov_b32 v140, 0x7fc0dead\n\tv_mov_b32 v141, 0x7fc0dead\n\tv_mov_b32 v142, 0x7fc0dead\n\tv_mov_b32 v143, 0x7fc0dead\n\tv_mov_b32 v144, 0x7fc0dead\n\tv_mov_b32 v145, 0x7fc0dead\n\tv_mov_b32 v146, 0x7fc0dead\n\tv_mov_b32 v147, 0x7fc0dead\n\tv_mov_b32 v148, 0x7fc0dead\n\tv_mov_b32 v149, 0x7fc0dead\n\tv_mov_b32 v150, 0x7fc0dead\n\tv_mov_b32 v151, 0x7fc0dead\n\tv_mov_b32 v152, 0x7fc0dead\n\tv_mov_b32 v153, 0x7fc0dead\n\tv_mov_b32 v154, 0x7fc0dead\n\tv_mov_b32 v155, 0x7fc0dead\n\tv_mov_b32 v156, 0x7fc0dead\n\tv_mov_b32 v157, 0x7fc0dead\n\tv_mov_b32 v158, 0x7fc0dead\n\tv_mov_b32 v159, 0x7fc0dead\n\tv_mov_b32 v160, 0x7fc0dead\n\tv_mov_b32 v161, 0x7fc0dead\n\tv_mov_b32 v162, 0x7fc0dead\n\tv_mov_b32 v163, 0x7fc0dead\n\tv_mov_b32 v164, 0x7fc0dead\n\tv_mov_b32 v165, 0x7fc0dead\n\tv_mov_b32 v166, 0x7fc0dead\n\tv_mov_b32 v167, 0x7fc0dead\n\tv_mov_b32 v168, 0x7fc0dead\n\tv_mov_b32 v169, 0x7fc0dead\n\tv_mov_b32 v170, 0x7fc0dead\n\tv_mov_b32 v171, 0x7fc0dead\n\tv_mov_b32 v172, 0x7fc0dead\n\tv_mov_b32 v173, 0x7fc0dead\n\tv_mov_b32 v174, 0x7fc0dead\n\tv_mov_b32 v175, 0x7fc0dead\n\tv_mov_b32 v176, 0x7fc0dead\n\tv_mov_b32 v177, 0x7fc0dead\n\tv_mov_b32 v178, 0x7fc0dead\n\tv_mov_b32 v179, 0x7fc0dead\n\tv_mov_b32 v180, 0x7fc0dead\n\tv_mov_b32 v181, 0x7fc0dead\n\tv_mov_b32 v182, 0x7fc0dead\n\tv_mov_b32 v183, 0x7fc0dead\n\tv_mov_b32 v184, 0x7fc0dead\n\tv_mov_b32 v185, 0x7fc0dead\n\tv_mov_b32 v186, 0x7fc0dead\n\tv_mov_b32 v187, 0x7fc0dead\n\tv_mov_b32 v188, 0x7fc0dead\n\tv_mov_b32 v189, 0x7fc0dead\n\tv_mov_b32 v190, 0x7fc0dead\n\tv_mov_b32 v191, 0x7fc0dead\n\tv_mov_b32 v192, 0x7fc0dead\n\tv_mov_b32 v193, 0x7fc0dead\n\tv_mov_b32 v194, 0x7fc0dead\n\tv_mov_b32 v195, 0x7fc0dead\n\tv_mov_b32 v196, 0x7fc0dead\n\tv_mov_b32 v197, 0x7fc0dead\n\tv_mov_b32 v198, 0x7fc0dead\n\tv_mov_b32 v199, 0x7fc0dead\n\tv_mov_b32 v200, 0x7fc0dead\n\tv_mov_b32 v201, 0x7fc0dead\n\tv_mov_b32 v202, 0x7fc0dead\n\tv_mov_b32 v203, 0x7fc0dead\n\tv_mov_b32 v204, 0x7fc0dead\n\tv_mov_b32 v205, 0x7fc0dead\n\tv_mov_b32 v206, 0x7fc0dead\n\tv_mov_b32 v207, 0x7fc0dead\n\tv_mov_b32 v208, 0x7fc0dead\n\tv_mov_b32 v209, 0x7fc0dead\n\tv_mov_b32 v210, 0x7fc0dead\n\tv_mov_b32 v211, 0x7fc0dead\n\tv_mov_b32 v212, 0x7fc0dead\n\tv_mov_b32 v213, 0x7fc0dead\n\tv_mov_b32 v214, 0x7fc0dead\n\tv_mov_b32 v215, 0x7fc0dead\n\tv_mov_b32 v216, 0x7fc0dead\n\tv_mov_b32 v217, 0x7fc0dead\n\tv_mov_b32 v218, 0x7fc0dead\n\tv_mov_b32 v219, 0x7fc0dead\n\tv_mov_b32 v220, 0x7fc0dead\n\tv_mov_b32 v221, 0x7fc0dead\n\tv_mov_b32 v222, 0x7fc0dead\n\tv_mov_b32 v223, 0x7fc0dead\n\tv_mov_b32 v224, 0x7fc0dead\n\tv_mov_b32 v225, 0x7fc0dead\n\tv_mov_b32 v226, 0x7fc0dead\n\tv_mov_b32 v227, 0x7fc0dead\n\tv_mov_b32 v228, 0x7fc0dead\n\tv_mov_b32 v229, 0x7fc0dead\n\tv_mov_b32 v230, 0x7fc0dead\n\tv_mov_b32 v231, 0x7fc0dead\n\tv_mov_b32 v232, 0x7fc0dead\n\tv_mov_b32 v233, 0x7fc0dead\n\tv_mov_b32 v234, 0x7fc0dead\n\tv_mov_b32 v235, 0x7fc0dead\n\tv_mov_b32 v236, 0x7fc0dead\n\tv_mov_b32 v237, 0x7fc0dead\n\tv_mov_b32 v238, 0x7fc0dead\n\tv_mov_b32 v239, 0x7fc0dead\n\tv_mov_b32 v240, 0x7fc0dead\n\tv_mov_b32 v241, 0x7fc0dead\n\tv_mov_b32 v242, 0x7fc0dead\n\tv_mov_b32 v243, 0x7fc0dead\n\tv_mov_b32 v244, 0x7fc0dead\n\tv_mov_b32 v245, 0x7fc0dead\n\tv_mov_b32 v246, 0x7fc0dead\n\tv_mov_b32 v247, 0x7fc0dead\n\tv_mov_b32 v248, 0x7fc0dead\n\tv_mov_b32 v249, 0x7fc0dead\n\tv_mov_b32 v250, 0x7fc0dead\n\tv_mov_b32 v251, 0x7fc0dead\n\tv_mov_b32 v252, 0x7fc0dead\n\tv_mov_b32 v253, 0x7fc0dead\n\tv_mov_b32 v254, 0x7fc0dead\n\tv_mov_b32 v255, 0x7fc0dead\n\tv_accvgpr_write_b32 a0, v0\n\tv_accvgpr_write_b32 a1, v0\n\tv_accvgpr_write_b32 a2, v0\n\tv_accvgpr_write_b32 a3, v0\n\tv_accvgpr_write_b32 a4, v0\n\tv_accvgpr_write_b32 a5, v0\n\tv_accvgpr_write_b32 a6, v0\n\tv_accvgpr_write_b32 a7, v0\n\tv_accvgpr_write_b32 a8, v0\n\tv_accvgpr_write_b32 a9, v0\n\tv_accvgpr_write_b32 a10, v0\n\tv_accvgpr_write_b32 a11, v0\n\tv_accvgpr_write_b32 a12, v0\n\tv_accvgpr_write_b32 a13, v0\n\tv_accvgpr_write_b32 a14, v0\n\tv_accvgpr_write_b32 a15, v0\n\tv_accvgpr_write_b32 a16, v0\n\tv_accvgpr_write_b32 a17, v0\n\tv_accvgpr_write_b32 a18, v0\n\tv_accvgpr_write_b32 a19, v0\n\tv_accvgpr_write_b32 a20, v0\n\tv_accvgpr_write_b32 a21, v0\n\tv_accvgpr_write_b32 a22, v0\n\tv_accvgpr_write_b32 a23, v0\n\tv_accvgpr_write_b32 a24, v0\n\tv_accvgpr_write_b32 a25, v0\n\tv_accvgpr_write_b32 a26, v0\n\tv_accvgpr_write_b32 a27, v0\n\tv_accvgpr_write_b32 a28, v0\n\tv_accvgpr_write_b32 a29, v0\n\tv_accvgpr_write_b32 a30, v0\n\tv_accvgpr_write_b32 a31, v0\n\tv_accvgpr_write_b32 a32, v0\n\tv_accvgpr_write_b32 a33, v0\n\tv_accvgpr_write_b32 a34, v0\n\tv_accvgpr_write_b32 a35, v0\n\tv_accvgpr_write_b32 a36, v0\n\tv_accvgpr_write_b32 a37, v0\n\tv_accvgpr_write_b32 a38, v0\n\tv_accvgpr_write_b32 a39, v0\n\tv_accvgpr_write_b32 a40, v0\n\tv_accvgpr_write_b32 a41, v0\n\tv_accvgpr_write_b32 a42, v0\n\tv_accvgpr_write_b32 a43, v0\n\tv_accvgpr_write_b32 a44, v0\n\tv_accvgpr_write_b32 a45, v0\n\tv_accvgpr_write_b32 a46, v0\n\tv_accvgpr_write_b32 a47, v0\n\tv_accvgpr_write_b32 a48, v0\n\tv_accvgpr_write_b32 a49, v0\n\tv_accvgpr_write_b32 a50, v0\n\tv_accvgpr_write_b32 a51, v0\n\tv_accvgpr_write_b32 a52, v0\n\tv_accvgpr_write_b32 a53, v0\n\tv_accvgpr_write_b32 a54, v0\n\tv_accvgpr_write_b32 a55, v0\n\tv_accvgpr_write_b32 a56, v0\n\tv_accvgpr_write_b32 a57, v0\n\tv_accvgpr_write_b32 a58, v0\n\tv_accvgpr_write_b32 a59, v0\n\tv_accvgpr_write_b32 a60, v0\n\tv_accvgpr_write_b32 a61, v0\n\tv_accvgpr_write_b32 a62, v0\n\tv_accvgpr_write_b32 a63, v0\n\tv_accvgpr_write_b32 a64, v0\n\tv_accvgpr_write_b32 a65, v0\n\tv_accvgpr_write_b32 a66, v0\n\tv_accvgpr_write_b32 a67, v0\n\tv_accvgpr_write_b32 a68, v0\n\tv_accvgpr_write_b32 a69, v0\n\tv_accvgpr_write_b32 a70, v0\n\tv_accvgpr_write_b32 a71, v0\n\tv_accvgpr_write_b32 a72, v0\n\tv_accvgpr_write_b32 a73, v0\n\tv_accvgpr_write_b32 a74, v0\n\tv_accvgpr_write_b32 a75, v0\n\tv_accvgpr_write_b32 a76, v0\n\tv_accvgpr_write_b32 a77, v0\n\tv_accvgpr_write_b32 a78, v0\n\tv_accvgpr_write_b32 a79, v0\n\tv_accvgpr_write_b32 a80, v0\n\tv_accvgpr_write_b32 a81, v0\n\tv_accvgpr_write_b32 a82, v0\n\tv_accvgpr_write_b32 a83, v0\n\tv_accvgpr_write_b32 a84, v0\n\tv_accvgpr_write_b32 a85, v0\n\tv_accvgpr_write_b32 a86, v0\n\tv_accvgpr_write_b32 a87, v0\n\tv_accvgpr_write_b32 a88, v0\n\tv_accvgpr_write_b32 a89, v0\n\tv_accvgpr_write_b32 a90, v0\n\tv_accvgpr_write_b32 a91, v0\n\tv_accvgpr_write_b32 a92, v0\n\tv_accvgpr_write_b32 a93, v0\n\tv_accvgpr_write_b32 a94, v0\n\tv_accvgpr_write_b32 a95, v0\n\tv_accvgpr_write_b32 a96, v0\n\tv_accvgpr_write_b32 a97, v0\n\tv_accvgpr_write_b32 a98, v0\n\tv_accvgpr_write_b32 a99, v0\n\tv_accvgpr_write_b32 a100, v0\n\tv_accvgpr_write_b32 a101, v0\n\tv_accvgpr_write_b32 a102, v0\n\tv_accvgpr_write_b32 a103, v0\n\tv_accvgpr_write_b32 a104, v0\n\tv_accvgpr_write_b32 a105, v0\n\tv_accvgpr_write_b32 a106, v0\n\tv_accvgpr_write_b32 a107, v0\n\tv_accvgpr_write_b32 a108, v0\n\tv_accvgpr_write_b32 a109, v0\n\tv_accvgpr_write_b32 a110, v0\n\tv_accvgpr_write_b32 a111, v0\n\tv_accvgpr_write_b32 a112, v0\n\tv_accvgpr_write_b32 a113, v0\n\tv_accvgpr_write_b32 a114, v0\n\tv_accvgpr_write_b32 a115, v0\n\tv_accvgpr_write_b32 a116, v0\n\tv_accvgpr_write_b32 a117, v0\n\tv_accvgpr_write_b32 a118, v0\n\tv_accvgpr_write_b32 a119, v0\n\tv_accvgpr_write_b32 a120, v0\n\tv_accvgpr_write_b32 a121, v0\n\tv_accvgpr_write_b32 a122, v0\n\tv_accvgpr_write_b32 a123, v0\n\tv_accvgpr_write_b32 a124, v0\n\tv_accvgpr_write_b32 a125, v0\n\tv_accvgpr_write_b32 a126, v0\n\tv_accvgpr_write_b32 a127, v0\n\tv_accvgpr_write_b32 a128, v0\n\tv_accvgpr_write_b32 a129, v0\n\tv_accvgpr_write_b32 a130, v0\n\tv_accvgpr_write_b32 a131, v0\n\tv_accvgpr_write_b32 a132, v0\n\tv_accvgpr_write_b32 a133, v0\n\tv_accvgpr_write_b32 a134, v0\n\tv_accvgpr_write_b32 a135, v0\n\tv_accvgpr_write_b32 a136, v0\n\tv_accvgpr_write_b32 a137, v0\n\tv_accvgpr_write_b32 a138, v0\n\tv_accvgpr_write_b32 a139, v0\n\tv_accvgpr_write_b32 a140, v0\n\tv_accvgpr_write_b32 a141, v0\n\tv_accvgpr_write_b32 a142, v0\n\tv_accvgpr_write_b32 a143, v0\n\tv_accvgpr_write_b32 a144, v0\n\tv_accvgpr_write_b32 a145, v0\n\tv_accvgpr_write_b32 a146, v0\n\tv_accvgpr_write_b32 a147, v0\n\tv_accvgpr_write_b32 a148, v0\n\tv_accvgpr_write_b32 a149, v0\n\tv_accvgpr_write_b32 a150, v0\n\tv_accvgpr_write_b32 a151, v0\n\tv_accvgpr_write_b32 a152, v0\n\tv_accvgpr_write_b32 a153, v0\n\tv_accvgpr_write_b32 a154, v0\n\tv_accvgpr_write_b32 a155, v0\n\tv_accvgpr_write_b32 a156, v0\n\tv_accvgpr_write_b32 a157, v0\n\tv_accvgpr_write_b32 a158, v0\n\tv_accvgpr_write_b32 a159, v0\n\tv_accvgpr_write_b32 a160, v0\n\tv_accvgpr_write_b32 a161, v0\n\tv_accvgpr_write_b32 a162, v0\n\tv_accvgpr_write_b32 a163, v0\n\tv_accvgpr_write_b32 a164, v0\n\tv_accvgpr_write_b32 a165, v0\n\tv_accvgpr_write_b32 a166, v0\n\tv_accvgpr_write_b32 a167, v0\n\tv_accvgpr_write_b32 a168, v0\n\tv_accvgpr_write_b32 a169, v0\n\tv_accvgpr_write_b32 a170, v0\n\tv_accvgpr_write_b32 a171, v0\n\tv_accvgpr_write_b32 a172, v0\n\tv_accvgpr_write_b32 a173, v0\n\tv_accvgpr_write_b32 a174, v0\n\tv_accvgpr_write_b32 a175, v0\n\tv_accvgpr_write_b32 a176, v0\n\tv_accvgpr_write_b32 a177, v0\n\tv_accvgpr_write_b32 a178, v0\n\tv_accvgpr_write_b32 a179, v0\n\tv_accvgpr_write_b32 a180, v0\n\tv_accvgpr_write_b32 a181, v0\n\tv_accvgpr_write_b32 a182, v0\n\tv_accvgpr_write_b32 a183, v0\n\tv_accvgpr_write_b32 a184, v0\n\tv_accvgpr_write_b32 a185, v0\n\tv_accvgpr_write_b32 a186, v0\n\tv_accvgpr_write_b32 a187, v0\n\tv_accvgpr_write_b32 a188, v0\n\tv_accvgpr_write_b32 a189, v0\n\tv_accvgpr_write_b32 a190, v0\n\tv_accvgpr_write_b32 a191, v0\n\tv_accvgpr_write_b32 a192, v0\n\tv_accvgpr_write_b32 a193, v0\n\tv_accvgpr_write_b32 a194, v0\n\tv_accvgpr_write_b32 a195, v0\n\tv_accvgpr_write_b32 a196, v0\n\tv_accvgpr_write_b32 a197, v0\n\tv_accvgpr_write_b32 a198, v0\n\tv_accvgpr_write_b32 a199, v0\n\tv_accvgpr_write_b32 a200, v0\n\tv_accvgpr_write_b32 a201, v0\n\tv_accvgpr_write_b32 a202, v0\n\tv_accvgpr_write_b32 a203, v0\n\tv_accvgpr_write_b32 a204, v0\n\tv_accvgpr_write_b32 a205, v0\n\tv_accvgpr_write_b32 a206, v0\n\tv_accvgpr_write_b32 a207, v0\n\tv_accvgpr_write_b32 a208, v0\n\tv_accvgpr_write_b32 a209, v0\n\tv_accvgpr_write_b32 a210, v0\n\tv_accvgpr_write_b32 a211, v0\n\tv_accvgpr_write_b32 a212, v0\n\tv_accvgpr_write_b32 a213, v0\n\tv_accvgpr_write_b32 a214, v0\n\tv_accvgpr_write_b32 a215, v0\n\tv_accvgpr_write_b32 a216, v0\n\tv_accvgpr_write_b32 a217, v0\n\tv_accvgpr_write_b32 a218, v0\n\tv_accvgpr_write_b32 a219, v0\n\tv_accvgpr_write_b32 a220, v0\n\tv_accvgpr_write_b32 a221, v0\n\tv_accvgpr_write_b32 a222, v0\n\tv_accvgpr_write_b32 a223, v0\n\tv_accvgpr_write_b32 a224, v0\n\tv_accvgpr_write_b32 a225, v0\n\tv_accvgpr_write_b32 a226, v0\n\tv_accvgpr_write_b32 a227, v0\n\tv_accvgpr_write_b32 a228, v0\n\tv_accvgpr_write_b32 a229, v0\n\tv_accvgpr_write_b32 a230, v0\n\tv_accvgpr_write_b32 a231, v0\n\tv_accvgpr_write_b32 a232, v0\n\tv_accvgpr_write_b32 a233, v0\n\tv_accvgpr_write_b32 a234, v0\n\tv_accvgpr_write_b32 a235, v0\n\tv_accvgpr_write_b32 a236, v0\n\tv_accvgpr_write_b32 a237, v0\n\tv_accvgpr_write_b32 a238, v0\n\tv_accvgpr_write_b32 a239, v0\n\tv_accvgpr_write_b32 a240, v0\n\tv_accvgpr_write_b32 a241, v0\n\tv_accvgpr_write_b32 a242, v0\n\tv_accvgpr_write_b32 a243, v0\n\tv_accvgpr_write_b32 a244, v0\n\tv_accvgpr_write_b32 a245, v0\n\tv_accvgpr_write_b32 a246, v0\n\tv_accvgpr_write_b32 a247, v0\n\tv_accvgpr_write_b32 a248, v0\n\tv_accvgpr_write_b32 a249, v0\n\tv_accvgpr_write_b32 a250, v0\n\tv_accvgpr_write_b32 a251, v0\n\tv_accvgpr_write_b32 a252, v0\n\tv_accvgpr_write_b32 a253, v0\n\tv_accvgpr_write_b32 a254, v0\n\tv_accvgpr_write_b32 a255, v0\n\ts_sleep 127\n\ts_sleep 127\n\ts_sleep 127\n\ts_sleep 127" ::: "v0", "v1", "v2", "v3", "v4", "v5", "v6", "v7", "v8", "v9", "v10", "v11", "v12", "v13", "v14", "v15", "v16", "v17", "v18", "v19", "v20", "v21", "v22", "v23", "v24", "v25", "v26", "v27", "v28", "v29", "v30", "v31", "v32", "v33", "v34", "v35", "v36", "v37", "v38", "v39", "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59", "v60", "v61", "v62", "v63", "v64", "v65", "v66", "v67", "v68", "v69", "v70", "v71", "v72", "v73", "v74", "v75", "v76", "v77", "v78", "v79", "v80", "v81", "v82", "v83", "v84", "v85", "v86", "v87", "v88", "v89", "v90", "v91", "v92", "v93", "v94", "v95", "v96", "v97", "v98", "v99", "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107", "v108", "v109", "v110", "v111", "v112", "v113", "v114", "v115", "v116", "v117", "v118", "v119", "v120", "v121", "v122", "v123", "v124", "v125", "v126", "v127", "v128", "v129", "v130", "v131", "v132", "v133", "v134", "v135", "v136", "v137", "v138", "v139", "v140", "v141", "v142", "v143", "v144", "v145", "v146", "v147", "v148", "v149", "v150", "v151", "v152", "v153", "v154", "v155", "v156", "v157", "v158", "v159", "v160", "v161", "v162", "v163", "v164", "v165", "v166", "v167", "v168", "v169", "v170", "v171", "v172", "v173", "v174", "v175", "v176", "v177", "v178", "v179", "v180", "v181", "v182", "v183", "v184", "v185", "v186", "v187", "v188", "v189", "v190", "v191", "v192", "v193", "v194", "v195", "v196", "v197", "v198", "v199", "v200", "v201", "v202", "v203", "v204", "v205", "v206", "v207", "v208", "v209", "v210", "v211", "v212", "v213", "v214", "v215", "v216", "v217", "v218", "v219", "v220", "v221", "v222", "v223", "v224", "v225", "v226", "v227", "v228", "v229", "v230", "v231", "v232", "v233", "v234", "v235", "v236", "v237", "v238", "v239", "v240", "v241", "v242", "v243", "v244", "v245", "v246", "v247", "v248", "v249", "v250", "v251", "v252", "v253", "v254", "v255", "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", "a10", "a11", "a12", "a13", "a14", "a15", "a16", "a17", "a18", "a19", "a20", "a21", "a22", "a23", "a24", "a25", "a26", "a27", "a28", "a29", "a30", "a31", "a32", "a33", "a34", "a35", "a36", "a37", "a38", "a39", "a40", "a41", "a42", "a43", "a44", "a45", "a46", "a47", "a48", "a49", "a50", "a51", "a52", "a53", "a54", "a55", "a56", "a57", "a58", "a59", "a60", "a61", "a62", "a63", "a64", "a65", "a66", "a67", "a68", "a69", "a70", "a71", "a72", "a73", "a74", "a75", "a76", "a77", "a78", "a79", "a80", "a81", "a82", "a83", "a84", "a85", "a86", "a87", "a88", "a89", "a90", "a91", "a92", "a93", "a94", "a95", "a96", "a97", "a98", "a99", "a100", "a101", "a102", "a103", "a104", "a105", "a106", "a107", "a108", "a109", "a110", "a111", "a112", "a113", "a114", "a115", "a116", "a117", "a118", "a119", "a120", "a121", "a122", "a123", "a124", "a125", "a126", "a127", "a128", "a129", "a130", "a131", "a132", "a133", "a134", "a135", "a136", "a137", "a138", "a139", "a140", "a141", "a142", "a143", "a144", "a145", "a146", "a147", "a148", "a149", "a150", "a151", "a152", "a153", "a154", "a155", "a156", "a157", "a158", "a159", "a160", "a161", "a162", "a163", "a164", "a165", "a166", "a167", "a168", "a169", "a170", "a171", "a172", "a173", "a174", "a175", "a176", "a177", "a178", "a179", "a180", "a181", "a182", "a183", "a184", "a185", "a186", "a187", "a188", "a189", "a190", "a191", "a192", "a193", "a194", "a195", "a196", "a197", "a198", "a199", "a200", "a201", "a202", "a203", "a204", "a205", "a206", "a207", "a208", "a209", "a210", "a211", "a212", "a213", "a214", "a215", "a216", "a217", "a218", "a219", "a220", "a221", "a222", "a223", "a224", "a225", "a226", "a227", "a228", "a229", "a230", "a231", "a232", "a233", "a234", "a235", "a236", "a237", "a238", "a239", "a240", "a241", "a242", "a243", "a244", "a245", "a246", "a247", "a248", "a249", "a250", "a251", "a252", "a253", "a254", "a255");
}

extern "C" int rft_poison_vgprs(void* stream) {
    hipLaunchKernelGGL(k_poison_vgprs, dim3(8192), dim3(64), 0, (hipStream_t)stream);
    return (int)hipGetLastError();
}

// 36 accumulator tiles stay live: ~154 VGPRs, three waves per SIMD at most -- two of its workgroups never fill a SIMD's register file
__global__ __launch_bounds__(256, 3) void k_f16_mfma_load(float* out, int iters) {
    f32x4 acc[36];
#pragma unroll
    for (int i = 0; i < 36; ++i) acc[i] = (f32x4){(float)threadIdx.x, (float)i, 1.f, 2.f};
    h8 a, b;
#pragma unroll
    for (int j = 0; j < 8; ++j) { a[j] = (_Float16)(0.001f * (threadIdx.x & 15) + j); b[j] = (_Float16)(0.002f * j + 1.f); }
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 36; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc[i], 0, 0, 0);
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 36; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    out[blockIdx.x * 256 + threadIdx.x] = s;
}

// blocks x 256 threads; `out` holds blocks * 256 floats.  iters = 60000 runs ~15 ms on MI355X.
extern "C" int rft_f16_mfma_load(int blocks, int iters, float* out, void* stream) {
    hipLaunchKernelGGL(k_f16_mfma_load, dim3(blocks), dim3(256), 0, (hipStream_t)stream, out, iters);
    return (int)hipGetLastError();
}

// one wave.  din [64][18]: (a, b) of the pair butterflies, then the 16 values of the transpose sum; fin [64][8]: the pool cell's blocks u, v.
// dout [64][11]: (a, b) after masks {16, 32} | {1, 2, 4} | {4, 2, 1}, the transpose total, the pooled (sm, sq) from zero, (sm, sq) of ReLU(u) from zero;
// fout [64][2]: (p0, p1); iout [64]: rf_transpose_slot16(lane)
__global__ __launch_bounds__(64) void k_lane_reduce_probe(const double* __restrict__ din, const float* __restrict__ fin, double* __restrict__ dout,
                                                          float* __restrict__ fout, int* __restrict__ iout) {
    const int lane = threadIdx.x;
    const double a = din[lane * 18], b = din[lane * 18 + 1];
    double* o = dout + lane * 11;
    double x = a, y = b;
    rf_xor_sum2<16, 32>(x, y);
    o[0] = x; o[1] = y;
    x = a; y = b;
    rf_xor_sum2<1, 4>(x, y);
    o[2] = x; o[3] = y;
    x = a; y = b;
    rf_xor_sum2<4, 1>(x, y);
    o[4] = x; o[5] = y;
    double v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = din[lane * 18 + 2 + i];
    o[6] = rf_transpose_sum16(v, lane);
    iout[lane] = rf_transpose_slot16(lane);
    f32x4 u4, v4;
#pragma unroll
    for (int r = 0; r < 4; ++r) { u4[r] = fin[lane * 8 + r]; v4[r] = fin[lane * 8 + 4 + r]; }
    float p0, p1;
    rf_pool_cell(u4, v4, p0, p1);
    fout[lane * 2] = p0; fout[lane * 2 + 1] = p1;
    double sm = 0.0, sq = 0.0;
    rf_pool_sums(p0, p1, sm, sq);
    o[7] = sm; o[8] = sq;
    sm = 0.0; sq = 0.0;
    rf_relu_sums(u4, sm, sq);
    o[9] = sm; o[10] = sq;
}

extern "C" int rft_lane_reduce_probe(const double* din, const float* fin, double* dout, float* fout, int* iout, void* stream) {
    hipLaunchKernelGGL(k_lane_reduce_probe, dim3(1), dim3(64), 0, (hipStream_t)stream, din, fin, dout, fout, iout);
    return (int)hipGetLastError();
}

// The workgroup reductions: 32 workgroups x 256 threads, each workgroup on its own inputs.  din [32][256][5]: column 0 = the K = 1 value, 1 .. 4 = the K = 4
// values; fin [32][256][2]: the float tree's value, the (non-negative) value of the maximum; lin [32][256]: the integer sum's value.
// dout [32][4][5]: the wave-order sums as thread k < K holds them (K = 1: thread 0) | all of them as the LAST thread reads them | 0.0 + the sums (thread 0) |
// the halving tree's red[0][:] in thread 0.  fout [32][3]: the float tree, the maximum in thread 0, in the last thread.  lout [32][2]: thread 0, last thread.
__global__ __launch_bounds__(256) void k_block_reduce_probe(const double* __restrict__ din, const float* __restrict__ fin, const long long* __restrict__ lin,
                                                            double* __restrict__ dout, float* __restrict__ fout, long long* __restrict__ lout) {
    __shared__ double w1[4][1], w4[4][4], t1[256][1], t4[256][4];
    __shared__ float tf[256][1], wm[4][1];
    __shared__ long long wl[4][1];
    const int t = threadIdx.x, b = blockIdx.x;
    const size_t e = (size_t)b * 256 + t;
    const double d1[1] = {din[e * 5]}, d4[4] = {din[e * 5 + 1], din[e * 5 + 2], din[e * 5 + 3], din[e * 5 + 4]};
    double* o = dout + (size_t)b * 20;
    rf_waves_put(w1, {wave_sum(d1[0])});
    rf_waves_put(w4, {wave_sum(d4[0]), wave_sum(d4[1]), wave_sum(d4[2]), wave_sum(d4[3])});
    rf_waves_put(wm, {wave_max(fin[e * 2 + 1])});
    rf_waves_put(wl, {wave_sum(lin[e])});
    if (t == 0) o[0] = rf_waves_sum(w1);
    if (t < 4) o[1 + t] = rf_waves_sum(w4, t);
    if (t == 255) {
        o[5] = rf_waves_sum(w1);
#pragma unroll
        for (int k = 0; k < 4; ++k) o[6 + k] = rf_waves_sum(w4, k);
    }
    if (t == 0) {
        o[10] = 0.0 + rf_waves_sum(w1);
#pragma unroll
        for (int k = 0; k < 4; ++k) o[11 + k] = 0.0 + rf_waves_sum(w4, k);
        fout[b * 3 + 1] = rf_waves_max(wm);
        lout[b * 2] = rf_waves_sum(wl);
    }
    if (t == 255) {
        fout[b * 3 + 2] = rf_waves_max(wm);
        lout[b * 2 + 1] = rf_waves_sum(wl);
    }
    rf_tree_sum(t1, d1);
    rf_tree_sum(t4, d4);
    rf_tree_sum(tf, {fin[e * 2]});
    if (t == 0) {
        o[15] = t1[0][0];
#pragma unroll
        for (int k = 0; k < 4; ++k) o[16 + k] = t4[0][k];
        fout[b * 3] = tf[0][0];
    }
}

extern "C" int rft_block_reduce_probe(const double* din, const float* fin, const long long* lin, double* dout, float* fout, long long* lout, void* stream) {
    hipLaunchKernelGGL(k_block_reduce_probe, dim3(32), dim3(256), 0, (hipStream_t)stream, din, fin, lin, dout, fout, lout);
    return (int)hipGetLastError();
}
