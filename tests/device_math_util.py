"""what tests/cpp/test_device_math.hip prints one line for: the functions of the shared host / device headers, the six that
are also compared with the host's libm first"""
FUNCTIONS = ["lm_sinf", "lm_cosf", "lm_atanf", "lm_acosf", "lm_expf", "lm_atan2f", "pf_roots2", "plane_from_sums",
             "plane_from_covariance", "rift_solve3", "rift_project", "rift_vote", "rift_vote_bins", "rift_norm", "rift_intensity",
             "sift_intensity", "sift_weight", "sift_response", "sift_dog", "sift_is_keypoint", "sym4_max_eigvec", "rigid_from_sums",
             "mat4_mul_f"]
