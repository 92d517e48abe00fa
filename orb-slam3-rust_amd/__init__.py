"""orb-slam3-rust_amd — MI355X-native (gfx950) hot path of jurmy24/orb-slam3-rust:
stereo ORB extract + match + triangulate and visual local bundle adjustment, as hand-written HIP
kernels behind the C ABI of include/orbx.h.  See DESIGN.md / INTEGRATION.md.

Import as `orb_slam3_rust_amd` (the shim at the repo root maps the hyphenated directory name).
"""
from . import dist, synth  # noqa: F401
from .api import (  # noqa: F401
    ABI_SYMBOLS, BA_OBS, BA_OBS32, BA_OBS32_STEREO, ba_obs_to_obs32, DMATCH, KEYPOINT, NN_RATIO, TH_HIGH, TH_LOW, CameraModel, FeatureSet, GlobalBAConfig, Handle,
    LocalBAConfigLM, OrbxError, StereoFrame, StereoProcessor, VisualBAProblemData, VisualBAResultData,
    VisualObservation, bf_match_crosscheck, descriptor_distance, flatten_ba_problem, load_library,
    solve_visual_ba, GlobalBAObservation, GlobalBAProblemData, GlobalBAResult, flatten_global_ba_problem, se3_inverse,
    solve_global_ba, OrbVocabulary, EurocDataset, png_decode_gray8, LocalInertialBAConfig, InertialVisualObs, ImuEdgeData, InertialBAProblemData,
    InertialBAResultData, flatten_inertial_ba_problem, solve_inertial_ba, MapSnapshot, local_bundle_adjustment, run_global_ba, KeyFrame, BaBatch,
    PnPConfig, PnPResult, PNP_RESULT, PNP_OK, PNP_NO_MODEL, PNP_TOO_FEW, PNP_OVER_MAX_N, solve_pnp_ransac, solve_pnp_ransac_detailed,
    PoseInertialConfig, PoseInertialResult, POSE_INERTIAL_RESULT, POSE_INERTIAL_OK, POSE_INERTIAL_TOO_FEW, POSE_INERTIAL_SINGULAR,
    pose_inertial_optimization, KeyFrameDatabase, LoopDetectorConfig, LoopCandidate, ConsistencyChecker, KFDB_SCORE_L1, KFDB_SCORE_DOT,
    KFDB_MAX_WORDS, TriangulationConfig, TriangulationResult, TRI_CREATED, TRI_SKIPPED, TRI_DLT_DEGENERATE, TRI_REJ_DEPTH, TRI_REJ_REPROJ1,
    TRI_REJ_REPROJ2, TRI_REJ_DIST, TRI_REJ_SCALE, TRI_BAD_INDEX, TRI_METHOD_DLT, TRI_METHOD_STEREO_CURRENT, TRI_METHOD_STEREO_NEIGHBOUR,
    TRI_MAX_NEIGHBOURS, FEATURE_NODE_NONE, TrackConfig, TrackFrameResult, TRACK_RESULT, TRACK_OK, TRACK_NO_MODEL,
    TRACK_TOO_FEW_CORRESPONDENCES, TRACK_TOO_FEW_INLIERS, TRACK_MOTION_MODEL, TRACK_LOCAL_MAP, TRACK_REF_RESULT, TrackReferenceResult,
    track_with_reference_kf, Sim3SolverConfig, Sim3Result, LoopVerifyConfig, VerifiedLoop, SIM3_RESULT, LOOP_VERIFY_RESULT, SIM3_OK, SIM3_NO_MODEL,
    LOOP_OK, LOOP_TOO_FEW_POINTS, LOOP_TOO_FEW_MATCHES, LOOP_TOO_FEW_PAIRS, LOOP_NO_MODEL, LOOP_TOO_FEW_INLIERS, LOOP_TOO_FEW_VERIFIED,
    LOOP_VERIFY_MAX_FEAT, MP_REFRESH_RECORD, MapPointRefresh, MapPointRefreshData, compute_sim3_ransac, compute_sim3_from_matches, verify_loop_candidate,
    MapPointStore, MAP_SOURCE_KEYFRAMES, MAP_SOURCE_SLOTS, MAP_CREATE_STEREO, MAP_CREATE_NEIGHBOURS, covisibility_lists, MapLocalBAResult, LoopCorrectConfig)
from .build import LIB_PATH, build  # noqa: F401
