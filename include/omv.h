/* omv.h — C ABI of the MI355X-native OpenMAVIS hot path (libomv_hip.so).
 *
 * Plain pointers and sizes only; no torch / OpenCV / Eigen types.  Every call is reentrant per
 * handle; a handle must not be used by two threads at once (the reference's extractors have the
 * same rule: one ORBextractor per camera thread, src/Frame.cc:1841-1862).  Device pointers are HIP
 * device memory; `stream` is a hipStream_t (NULL = the default stream).  Functions return an
 * omv_status; nothing throws across the ABI.
 *
 * Each entry point names the reference interface it replaces (file:line in the reference).
 */
#ifndef OMV_H
#define OMV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int omv_status;
#define OMV_OK 0
#define OMV_ERR_ARG 1          /* bad argument (NULL, size out of range)                        */
#define OMV_ERR_HIP 2          /* a HIP runtime call failed                                     */
#define OMV_ERR_CAPACITY 3     /* a device-side capacity was exceeded (reported, never silent)  */
#define OMV_ERR_NO_DEVICE 4    /* no HIP device visible: there is no CPU fallback               */

/* ------------------------------------------------------------------------------------------------
 * ORB extraction — replaces ORBextractor::ORBextractor (src/ORBextractor.cc:351-414) and
 * ORBextractor::operator() (include/ORBextractor.h:33-38, src/ORBextractor.cc:987-1071).
 * ---------------------------------------------------------------------------------------------- */
typedef struct omv_orb_params {
    int nfeatures;      /* ORBextractor.nFeatures                                  */
    float scale_factor; /* ORBextractor.scaleFactor (1.2)                          */
    int nlevels;        /* ORBextractor.nLevels (8)                                */
    int ini_th_fast;    /* ORBextractor.iniThFAST                                  */
    int min_th_fast;    /* ORBextractor.minThFAST                                  */
} omv_orb_params;

/* cv::KeyPoint fields the reference reads (pt, size, angle, response, octave); 24 bytes. */
typedef struct omv_kp {
    float x, y, size, angle, response;
    int32_t octave;
} omv_kp;

typedef struct omv_orb omv_orb;

/* Create an extractor for images of width x height (u8), batching up to max_images per call. */
omv_status omv_orb_create(const omv_orb_params *params, int width, int height, int max_images,
                          omv_orb **out);
omv_status omv_orb_destroy(omv_orb *orb);

/* Test hook (no reference counterpart): the device replica of libstdc++'s std::sort that the octree
 * uses for DistributeOctTree's compareNodes order (src/ORBextractor.cc:482-494, :629-632), on one
 * array of n <= 2048 (k1, k2) pairs with k1 >= 0, 0 <= k2 < 2^20 (device memory); perm receives the
 * original indices in sorted order. */
omv_status omv_selftest_node_sort(const int *k1, const int *k2, int n, int *perm, void *stream);

/* Upper bound on keypoints one image can produce (output row capacity N_max).  The reference can
 * return up to quota+2 keypoints per level (DistributeOctTree :673 stops at >= N). */
int omv_orb_max_keypoints(const omv_orb *orb);

/* The ORBextractor getters (include/ORBextractor.h:40-50): nlevels floats each, host memory. */
omv_status omv_orb_scale_tables(const omv_orb *orb, float *scale, float *inv_scale, float *sigma2,
                                float *inv_sigma2);

/* Batched ORBextractor::operator() over n_images device-resident images.
 *   images      device, image i at images + i*image_stride, rows `pitch` bytes apart
 *   lapping     host, 2 ints per image: [x0, x1] (vLappingArea)
 *   kps         device, [n_images][N_max] omv_kp
 *   desc        device, [n_images][N_max][32] u8
 *   n_out       device, [n_images] keypoint count (rows of kps/desc that are valid)
 *   mono_index  device, [n_images] return value of operator() (monoIndex)
 * Output order per image is the reference's: non-lapping keypoints from the front, lapping ones
 * from the back in reverse, level by level.  Asynchronous on `stream`. */
omv_status omv_orb_extract_batch(omv_orb *orb, int n_images, const uint8_t *images, size_t image_stride,
                                 size_t pitch, const int *lapping, omv_kp *kps, uint8_t *desc, int *n_out,
                                 int *mono_index, void *stream);

/* Synchronous host-memory convenience used by the ORBextractor::operator() adapter: stages one
 * image H2D, extracts, copies back.  Returns monoIndex in *mono_index and the count in *n_out. */
omv_status omv_orb_extract_host(omv_orb *orb, const uint8_t *image, size_t pitch, int lap0, int lap1,
                                omv_kp *kps, uint8_t *desc, int *n_out, int *mono_index);

/* Optional extra output of the following omv_orb_extract_batch calls: per output row (the omv_kp layout
 * [image][N_max]) OpenCV ORB's Harris response (orb.cpp HarrisResponses, blockSize 7, k 0.04) at the keypoint's
 * level position -- the north star's "Harris score".  The reference never computes it (its HARRIS_SCORE is a dead
 * enum, include/ORBextractor.h:24; KeyPoint::response stays FAST's cornerScore).  NULL (default) disables it. */
omv_status omv_orb_set_harris(omv_orb *orb, float *harris);

/* Device-side error word of the last batch (OMV_ERR_CAPACITY if a bound was hit); syncs the stream. */
omv_status omv_orb_last_error(omv_orb *orb);

/* Per-stage device time (HIP events on the launch stream) for measurement: stages are
 * 0 pyramid, 1 FAST cells, 2 octree, 3 orientation + GaussianBlur 7x7 at the samples + descriptor.  omv_orb_stage_ms
 * syncs, returns the accumulated milliseconds since the last reset and the number of timed batches. */
omv_status omv_orb_enable_timing(omv_orb *orb, int on);
omv_status omv_orb_stage_ms(omv_orb *orb, double *ms4, long long *calls, int reset);

/* Measurement: FAST candidates (the octree's input) and distributed keypoints of the last batch, summed over its
 * images (synchronous read-back). */
omv_status omv_orb_last_counts(omv_orb *orb, long long *n_candidates, long long *n_keypoints);

/* Debug/parity hooks: copy pyramid level `level` of image `img` of the last batch to host. */
omv_status omv_orb_debug_level(omv_orb *orb, int img, int level, uint8_t *out, int *w, int *h);

/* ------------------------------------------------------------------------------------------------
 * Hamming matching on multi-camera frames
 *
 * Frame layout (device): keypoints/descriptors padded per camera block, kps [frame][cam][kp_cap],
 * desc [frame][cam][kp_cap][32], n_kp [frame][cam] (the extractor's batched output as-is).  Block 0
 * is the left camera, block 1 the right camera, blocks >= 2 side cameras — the reference's
 * [L|R|SL|SR] concatenation (src/Frame.cc:1936-1939) generalised to n_cams.  A keypoint "slot" is
 * cam * kp_cap + i; per-slot arrays (kp_to_mp, occupancy) are [frame][n_cams * kp_cap].
 * ---------------------------------------------------------------------------------------------- */
typedef struct omv_frame_geom {
    int n_cams;
    float min_x, max_x;  /* Frame::mnMinX/mnMaxX (bounds of imLeft, shared by all cameras, Frame.cc:1875) */
    float min_y, max_y;
    int nlevels;
    float scale_factors[16]; /* Frame::mvScaleFactors                                              */
    /* GeometricCamera type per camera block (Frame::mpCamera, mpCamera2, ...): OMV_CAM_KB8 (0, the
     * zero-initialised default) or OMV_CAM_PINHOLE.  The projection searches project with it:
     * SearchByProjection(F, LastF) block 0 (ORBmatcher.cc:2022, :2134), Fuse / SearchByProjection(KF, Sim3) /
     * SearchByProjection(F, KF) the job's block (:1536, :1710, :710, :2443). */
    int cam_model[8];
} omv_frame_geom;

/* Local map points projected into a frame (the MapPoint fields SearchByProjection reads after
 * Frame::isInFrustum, src/ORBmatcher.cc:33-60).  Device SoA: per-point arrays are [frame][M],
 * per-camera arrays [frame][M][n_cams]. */
typedef struct omv_mp_view {
    const uint8_t *desc;      /* [M][32] MapPoint::GetDescriptor()                                  */
    const float *proj_x;      /* [M][n_cams] mTrackProjX / XR / XSL / XSR ...                       */
    const float *proj_y;      /* [M][n_cams]                                                        */
    const float *view_cos;    /* [M][n_cams] mTrackViewCos*                                         */
    const int32_t *level;     /* [M][n_cams] mnTrackScaleLevel* (-1 = none)                         */
    const uint8_t *in_view;   /* [M][n_cams] mbTrackInView*                                         */
    const float *track_depth; /* [M] mTrackDepth                                                    */
    const uint8_t *is_bad;    /* [M] MapPoint::isBad()                                              */
    const uint8_t *has_obs;   /* [M] Observations() > 0                                             */
} omv_mp_view;

typedef struct omv_matcher omv_matcher;

/* Workspace for up to max_frames frames of n_cams blocks x kp_cap keypoints and max_mps points. */
omv_status omv_matcher_create(int max_frames, int n_cams, int kp_cap, int max_mps, omv_matcher **out);
omv_status omv_matcher_destroy(omv_matcher *m);

/* Frame::AssignFeaturesToGrid (src/Frame.cc:541-582) for n_frames frames: per camera a 64x48 grid
 * (cell = ix*48 + iy) of ascending keypoint indices, kept in the handle for the searches below. */
omv_status omv_matcher_assign_grid(omv_matcher *m, int n_frames, const omv_frame_geom *geom, const omv_kp *kps,
                                   const int *n_kp, void *stream);
/* Copy one camera's grid to host: cell_start [64*48+1], idx [kp_cap]. Syncs. */
omv_status omv_matcher_grid_debug(omv_matcher *m, int frame, int cam, int32_t *cell_start, int32_t *idx);

/* ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th, bFarPoints, thFarPoints)
 * (src/ORBmatcher.cc:23-340) on n_frames frames with the grid of the last assign_grid call.
 *   l2r / r2l     [frame][kp_cap] mvLeftToRightMatch / mvRightToLeftMatch (block-local indices, -1 none)
 *   kp_occ_init   [frame][slots] 1 where F.mvpMapPoints[slot] is already a point with observations
 *                 (may be NULL = none)
 *   kp_to_mp      [frame][slots] in/out: map point index assigned to each keypoint (F.mvpMapPoints)
 *   n_matches     [frame] the return value
 * Exactly the reference's sequential semantics: earlier points claim keypoints first, a failed
 * ratio test skips the point's remaining cameras, th scales only the left-camera window. */
omv_status omv_matcher_search_projection(omv_matcher *m, int n_frames, const omv_frame_geom *geom, const omv_kp *kps,
                                         const uint8_t *desc, const int *n_kp, const omv_mp_view *mps, int M, float th,
                                         int far_points, float th_far, float nnratio, const int32_t *l2r,
                                         const int32_t *r2l, const uint8_t *kp_occ_init, int32_t *kp_to_mp,
                                         int *n_matches, void *stream);
/* Copy the candidate records of the last search_projection call (n_frames frames, M points) to host: out
 * [n_frames][M][n_cams][16] words, idx | dist << 16 | octave << 25 | bit 31 valid (bit 30 of word 0: the window held
 * more than 16 unblocked candidates).  Only (point, camera) slots in view with a valid predicted level have a record;
 * the other slots' words are unspecified. Syncs. */
omv_status omv_matcher_records_debug(omv_matcher *m, int n_frames, int M, uint32_t *out);

/* Lapping-area stereo candidates of Frame::ComputeMultiFishEyeMatches (src/Frame.cc:1461-1491):
 * knnMatch(k=2) of camera-0 rows [mono0, n0) against camera-1 rows [mono1, n1), Lowe ratio
 * d0 < ratio * d1.  Writes l2r/r2l [frame][kp_cap] (later left index wins a shared right keypoint).
 * The KannalaBrandt8::TriangulateMatches depth check that follows in the reference is not applied. */
omv_status omv_matcher_stereo_lapping(omv_matcher *m, int n_frames, const uint8_t *desc, const int *n_kp,
                                      const int *mono, double ratio, int32_t *l2r, int32_t *r2l, void *stream);

/* The depth check of Frame::ComputeMultiFishEyeMatches (src/Frame.cc:1488-1512) on the pairs
 * omv_matcher_stereo_lapping left in l2r: KannalaBrandt8::TriangulateMatches(mpCamera2, kpL, kpR,
 * mRlr, mtlr, sigma2[octL], sigma2[octR]) > 1e-4 keeps a pair (l2r / r2l [frame][kp_cap], the later
 * left index wins on r2l), writes mvDepth of the left keypoints (depth [frame][kp_cap], -1 elsewhere)
 * and mvStereo3Dpoints (p3d [frame][kp_cap][3]); failures clear l2r.  kps: [frame][n_cams][kp_cap]
 * (block 0 = left, 1 = right).  cams: host [2][8] (L, R); Rlr / tlr / level_sigma2: host. */
omv_status omv_matcher_stereo_triangulate(omv_matcher *m, int n_frames, int n_cams, int kp_cap, const omv_kp *kps,
                                          const int *n_kp, const int *mono, const float *cams, const float *Rlr,
                                          const float *tlr, const float *level_sigma2, int nlevels, int32_t *l2r,
                                          int32_t *r2l, float *depth, float *p3d, void *stream);

/* Device-side error word (OMV_ERR_CAPACITY if a bound was hit) since the last call; syncs. */
omv_status omv_matcher_last_error(omv_matcher *m);

/* Per-stage device time: 0 grid, 1 lapping knn, 2 projection candidates, 3 claim resolution. */
omv_status omv_matcher_enable_timing(omv_matcher *m, int on);
omv_status omv_matcher_stage_ms(omv_matcher *m, double *ms4, int reset);

/* cv::BFMatcher(NORM_HAMMING).knnMatch(k=2) (src/Frame.cc:1483) over n_pairs independent sets:
 * query [pair][q_cap][32] with nq[pair] rows, train [pair][t_cap][32] with nt[pair] rows.
 * idx2/dist2 [pair][q_cap][2]: two nearest train rows, first index wins ties; -1 / INT32_MAX when
 * fewer than 1 / 2 train rows exist. */
omv_status omv_bf_knn2(int n_pairs, const uint8_t *query, int q_cap, const int *nq, const uint8_t *train, int t_cap,
                       const int *nt, int32_t *idx2, int32_t *dist2, void *stream);
/* Which kernel omv_bf_knn2 takes at this shape, under the OMV_KNN / OMV_KNN_IDX_LIMIT test knobs: 1 the matrix-core
 * kernel, 0 the lane kernel (always, once t_cap reaches the 2^16 rows the packed key cannot index).  Launches nothing. */
int omv_bf_knn2_path(int n_pairs, int q_cap, int t_cap);

/* ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono)
 * (src/ORBmatcher.cc:1985-2413, ComputeThreeMaxima :2537-2573): motion-model matching of the last
 * frame's tracked map points, multi-camera branch, generalised to n_cams blocks (block 1 searched at
 * Trl * x projected with the LEFT camera model, blocks >= 2 at the left projection — both as in the
 * reference), rotation-consistency filter when check_ori. */
typedef struct omv_se3f {          /* Sophus::SE3f: unit quaternion (x, y, z, w) and translation */
    float q[4];
    float t[3];
} omv_se3f;

typedef struct omv_last_frame {    /* device SoA per LastFrame keypoint slot s = cam * last_cap + i */
    const float *pos;              /* [frame][S][3] mvpMapPoints[s]->GetWorldPos()                  */
    const uint8_t *desc;           /* [frame][S][32] GetDescriptor()                                */
    const uint8_t *valid;          /* [frame][S] mvpMapPoints[s] && !mvbOutlier[s]                  */
    const uint8_t *has_obs;        /* [frame][S] Observations() > 0                                 */
    const omv_kp *kps;             /* [frame][S] LastFrame keypoint s (octave, angle)               */
    int S;                         /* slots per last frame (n_cams * last_cap), <= the matcher's max_mps */
} omv_last_frame;

/* cams: host [n_cams][8] camera parameters (block 0's, of type geom->cam_model[0], are used for every
 * projection, as the reference's CurrentFrame.mpCamera);
 * Tcw / Tlw: device [n_frames] current / last block-0 poses; Trl: host, block 1 from block 0;
 * kp_to_mp [frame][n_cams*kp_cap] in/out receives last-frame slots; n_matches [frame] (device). */
omv_status omv_matcher_search_last_frame(omv_matcher *m, int n_frames, const omv_frame_geom *geom, const omv_kp *kps,
                                         const uint8_t *desc, const int *n_kp, const float *cams, const omv_se3f *Tcw,
                                         const omv_se3f *Tlw, const omv_se3f *Trl, const omv_last_frame *last, float th,
                                         int bMono, float mb, int check_ori, const uint8_t *kp_occ_init,
                                         int32_t *kp_to_mp, int32_t *n_matches, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Keyframe-side projection searches: map points projected into one camera block of a
 * keyframe (or frame) of the last omv_matcher_assign_grid batch and matched by Hamming distance in the
 * GetFeaturesInArea window.  One call runs a list of jobs; a job = (keyframe, camera block, pose, a run
 * of map points).  Modes:
 *   OMV_KF_FUSE       ORBmatcher::Fuse(KF, vpMapPoints, th, cameraID) (src/ORBmatcher.cc:1458-1647):
 *                     depth / IsInImage / distance-invariance / 60-degree viewing tests, PredictScale,
 *                     KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:771-834), levels [pred-1, pred], the
 *                     chi2 reprojection gate (stereo 7.8 on block 0 where mvuRight >= 0, else 5.99), best
 *                     by (distance, window order) from 256, accepted at <= TH_LOW.  The caller applies
 *                     the Replace / AddObservation of each accepted (point, keypoint) in list order.
 *   OMV_KF_FUSE_SIM3  ORBmatcher::Fuse(KF, Scw, vpPoints, th, vpReplacePoint) (:1649-1769), one job per
 *                     camera block: no distance / viewing tests, no gate, best from INT_MAX.
 *   OMV_KF_SBP_SIM3   ORBmatcher::SearchByProjection(KF, Siw, vpPoints[, vpPointsKFs], vpMatched, th,
 *                     ratioHamming, cameraID) (:668-776, :778-893): keypoints matched before (kp_match
 *                     >= 0, initially and by earlier points of the job) are skipped, accepted at
 *                     <= TH_LOW * ratioHamming and claimed in kp_match.
 *   OMV_KF_SBP_FRAME  ORBmatcher::SearchByProjection(Frame&, KF, sAlreadyFound, th, ORBdist)
 *                     (:2415-2535): the "keyframe" of the job is the current frame (inclusive mnMinX..mnMaxX
 *                     bounds, Frame::GetFeaturesInArea with levels [pred-1, pred+1]), no viewing test,
 *                     claims in kp_match, accepted at <= ORBdist; with check_ori the rotation-histogram
 *                     filter (ComputeThreeMaxima, :2537-2573) un-claims matches outside the three top bins.
 * Jobs on the same keyframe / frame run in job order (claims carry over), others in parallel.  The
 * caller leaves out of a job's list the points the reference skips before projecting (isBad(),
 * IsInKeyFrame(pKF), spAlreadyFound / sAlreadyFound) and passes each job's camera pose as the
 * reference composes it (GetPose / GetRightPose / ..., SE3f(Siw.rotationMatrix(), Siw.translation() /
 * Siw.scale()), GetRelativePoseTrl() * Tlw, CurrentFrame.GetPose()).
 * ---------------------------------------------------------------------------------------------- */
enum { OMV_KF_FUSE = 0, OMV_KF_FUSE_SIM3 = 1, OMV_KF_SBP_SIM3 = 2, OMV_KF_SBP_FRAME = 3 };

typedef struct omv_kf_search_job {
    int kf;                /* keyframe / frame index in the assign_grid batch */
    int cam;               /* cameraID: the camera block searched */
    omv_se3f Tcw;          /* world -> camera block `cam` */
    float Ow[3];           /* that camera's centre (the distance / viewing tests) */
    int mp_start, mp_count;   /* the job's entries [mp_start, mp_start + mp_count) of mp_list; jobs tile
                                 mp_list in order */
} omv_kf_search_job;

typedef struct omv_kf_mps {        /* device map-point table */
    const float *pos;              /* [M][3] GetWorldPos()                                           */
    const float *normal;           /* [M][3] GetNormal()                                             */
    const float *min_dist;         /* [M] mfMinDistance (GetMinDistanceInvariance = 0.8f * it)      */
    const float *max_dist;         /* [M] mfMaxDistance (GetMaxDistanceInvariance = 1.2f * it)      */
    const uint8_t *desc;           /* [M][32] GetDescriptor()                                        */
} omv_kf_mps;

typedef struct omv_kf_search_params {
    int mode;                      /* OMV_KF_*                                                       */
    float th;                      /* window radius factor (th * mvScaleFactors[pred])                */
    float max_dist;                /* acceptance: best <= max_dist (TH_LOW, TH_LOW * ratio, ORBdist) */
    float bf;                      /* KeyFrame::mbf (OMV_KF_FUSE stereo gate)                         */
    const float *uright;           /* device [n_kf][kp_cap] mvuRight of block 0 (OMV_KF_FUSE) or NULL */
    float inv_level_sigma2[16];    /* mvInvLevelSigma2                                               */
    float log_scale_factor;        /* mfLogScaleFactor                                               */
    int n_levels;                  /* mnScaleLevels                                                  */
    float cams[8][8];              /* camera parameters per block (KB8 fx fy cx cy k1..k4 / Pinhole fx fy cx cy;
                                      the type is geom->cam_model[block])                             */
    int check_ori;                 /* OMV_KF_SBP_FRAME: mbCheckOrientation                           */
    const float *mp_angle;         /* device [n_entries]: pKF->mvKeysUn[i].angle per entry (check_ori) */
} omv_kf_search_params;

/* jobs: host [n_jobs] (validated, then copied to the handle); mp_list: device [n_entries] map-point table rows; kp_match: device
 * [n_kf][n_cams * kp_cap] slot claims (-1 free, else the claiming table row; in/out, claim modes only,
 * may be NULL otherwise); best_idx / best_dist: device [n_entries] — the chosen keypoint as the
 * keyframe's N-index (camera offset + index in its block; -1 if the point was rejected or nothing
 * qualified) and its distance (Fuse modes: the scan's best even above the threshold; claim modes: the
 * accepted match only); n_matches: device [n_jobs] the reference's return value per job. */
omv_status omv_matcher_search_kf(omv_matcher *m, int n_kf, const omv_frame_geom *geom, const omv_kp *kps,
                                 const uint8_t *desc, const int *n_kp, int n_jobs, const omv_kf_search_job *jobs,
                                 int n_entries, const int32_t *mp_list, const omv_kf_mps *mps,
                                 const omv_kf_search_params *p, int32_t *kp_match, int32_t *best_idx,
                                 int32_t *best_dist, int32_t *n_matches, void *stream);

/* ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, S12, th) (src/ORBmatcher.cc:1771-1983) for a list of
 * keyframe pairs of the last omv_matcher_assign_grid batch.  Side 1 of a job = the pKF1 keypoints i1 whose
 * map point the reference projects (GetMapPointMatches()[i1] set, !vbAlreadyMatched1[i1], !isBad()), as
 * (kp1 = i1, the N-index, mp1 = its map-point table row); side 2 likewise for pKF2.  Each side-1 point goes
 * through T1w then S21 into pKF2, each side-2 point through T2w then S12 into pKF1; both use the pinhole
 * formula with pKF1's fx fy cx cy (as the reference), IsInImage, the distance invariance on |p3Dc|,
 * PredictScale, KeyFrame::GetFeaturesInArea (camera block 0) at levels [pred-1, pred], the strict-< best,
 * kept at <= TH_HIGH; then the agreement check vnMatch2[vnMatch1[i1]] == i1.  A side's kp entries must be
 * distinct within a job. */
typedef struct omv_sim3f {         /* Sophus::Sim3f: RxSO3 quaternion (x, y, z, w; |q|^2 = scale), translation */
    float q[4];
    float t[3];
    float scale;                   /* S.scale() as the caller's Sophus computes it (q.squaredNorm())          */
} omv_sim3f;

typedef struct omv_sim3_job {
    int kf1, kf2;                  /* keyframes of the assign_grid batch                                       */
    omv_se3f T1w, T2w;             /* pKF1->GetPose(), pKF2->GetPose()                                         */
    omv_sim3f S12, S21;            /* S12 and S12.inverse()                                                    */
    float fx, fy, cx, cy;          /* pKF1->fx, fy, cx, cy                                                     */
    int start1, count1;            /* the job's run of the side-1 list (runs tile the list in order)          */
    int start2, count2;            /* the job's run of the side-2 list                                         */
} omv_sim3_job;

/* jobs: host [n_jobs]; kp1 / mp1: device [n1]; kp2 / mp2: device [n2]; mps: pos, min_dist, max_dist, desc
 * (normal unused); th: the radius factor; match12: device [n1] the pKF2 keypoint (N-index) matched to each
 * side-1 entry (vpMatches12[i1] = vpMapPoints2[match12]) or -1; n_found: device [n_jobs] the return value. */
omv_status omv_matcher_search_by_sim3(omv_matcher *m, int n_kf, const omv_frame_geom *geom, const omv_kp *kps,
                                      const uint8_t *desc, const int *n_kp, int n_jobs, const omv_sim3_job *jobs,
                                      int n1, const int32_t *kp1, const int32_t *mp1, int n2, const int32_t *kp2,
                                      const int32_t *mp2, const omv_kf_mps *mps, float th, float log_scale_factor,
                                      int n_levels, int32_t *match12, int32_t *n_found, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Frame::isInFrustum (src/Frame.cc:736-826; the multi-camera isInFrustumChecks, :1529-1653) with
 * MapPoint::PredictScale (src/MapPoint.cc:624-637) and KannalaBrandt8::project(Vector3f)
 * (src/CameraModels/KannalaBrandt8.cpp:48-67), for every local map point of every frame — the loop
 * of Tracking::SearchLocalPoints.  Writes the projection fields SearchByProjection reads.
 * ---------------------------------------------------------------------------------------------- */
/* GeometricCamera subclasses (src/CameraModels): KannalaBrandt8 (KannalaBrandt8.cpp) and Pinhole (Pinhole.cpp) */
#define OMV_CAM_KB8 0
#define OMV_CAM_PINHOLE 1

typedef struct omv_rig {
    int n_cams;
    float cam[8][8];               /* KannalaBrandt8 mvParameters per camera block                 */
    float R_cl[8][9], t_cl[8][3];  /* camera block c from block 0: mTrl / mTsll / mTsrl (c=0: I, 0) */
    float t_lc[8][3];              /* translation of the inverse: mTlr / mTlsl / mTlsr (c=0: 0)     */
    float min_x, max_x, min_y, max_y;  /* mnMinX .. mnMaxY                                          */
    float log_scale_factor;        /* mfLogScaleFactor                                              */
    int n_levels;                  /* mnScaleLevels                                                 */
    int model[8];                  /* camera model per block: OMV_CAM_KB8 (0, the default of a
                                      zero-initialised rig) or OMV_CAM_PINHOLE (cam[c][0..3] = fx fy cx cy) */
} omv_rig;

typedef struct omv_frame_pose {   /* block-0 camera: mRcw, mtcw and the inverse mRwc, mOw */
    float Rcw[9], tcw[3], Rwc[9], Ow[3];
} omv_frame_pose;

typedef struct omv_mp_world {     /* device SoA, [frame][M] */
    const float *pos;              /* [M][3] GetWorldPos()                                          */
    const float *normal;           /* [M][3] GetNormal()                                            */
    const float *min_dist;         /* [M] mfMinDistance                                             */
    const float *max_dist;         /* [M] mfMaxDistance                                             */
} omv_mp_world;

typedef struct omv_mp_track {     /* outputs, same layout as omv_mp_view */
    float *proj_x, *proj_y;        /* [M][n_cams] -1 when not in view (reset like the reference)    */
    float *view_cos;               /* [M][n_cams] written when in view                              */
    int32_t *level;                /* [M][n_cams] predicted level, -1 when not in view              */
    uint8_t *in_view;              /* [M][n_cams]                                                   */
    float *track_depth;            /* [M] block-0 distance, written only when block 0 sees the point */
} omv_mp_track;

/* poses: device [n_frames]; n_in_view (optional, device [n_frames], accumulated): points for which
 * isInFrustum returned true. */
omv_status omv_frustum(int n_frames, const omv_frame_pose *poses, const omv_rig *rig, const omv_mp_world *mp, int M,
                       float viewing_cos_limit, const omv_mp_track *out, int32_t *n_in_view, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Local inertial bundle adjustment — replaces the optimisation inside Optimizer::LocalInertialBA
 * (src/Optimizer.cc:2728-3385): EdgeMono / EdgeInertial / EdgeGyroRW / EdgeAccRW
 * (src/G2oTypes.cc, include/G2oTypes.h:283-633), g2o's Levenberg-Marquardt
 * (Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:61-169) with the landmark Schur
 * complement (block_solver.hpp:353-486).  The host adapter flattens the KeyFrame/MapPoint graph
 * (window selection, vertex ids, edge creation stay host-side, :2740-3267) into this problem and
 * writes the state back unless status == OMV_LBA_FAIL (the reference's FAIL guard, :3317-3321).
 * ---------------------------------------------------------------------------------------------- */
/* Per inertial edge: IMU::Preintegrated members in float, in this order:
 *   dR[9] dV[3] dP[3] JRg[9] JVg[9] JVa[9] JPg[9] JPa[9] b[6] (bax bay baz bwx bwy bwz) dT[1] C[225]
 * (3x3 / 15x15 row-major).  Information matrices are derived from C like EdgeInertial's ctor. */
#define OMV_PREINT_FLOATS 292
#define OMV_LBA_OK 0
#define OMV_LBA_FAIL 1   /* (2*err < err_end || isnan) && !bLarge: the reference discards the result */

typedef struct omv_lba_problem {
    int n_cams;
    const float *cam;          /* [n_cams][8] KannalaBrandt8 mvParameters: fx fy cx cy k1 k2 k3 k4 */
    const double *Rcb, *tcb;   /* [n_cams][9] row-major, [n_cams][3]: body -> camera (ImuCamPose) */
    const double *Rbc, *tbc;   /* [n_cams][9], [n_cams][3]: camera -> body */
    int n_kf;                  /* KeyFrame vertices; the first n_opt are optimisable, the rest fixed */
    int n_opt;
    const uint8_t *kf_imu;     /* [n_kf] KeyFrame::bImu: velocity / gyro / acc bias vertices exist */
    double *Rwb, *twb;         /* [n_kf][9], [n_kf][3] body pose (in/out) */
    double *Rcw, *tcw;         /* [n_kf][n_cams][9], [n_kf][n_cams][3] camera poses (in/out) */
    double *vel, *bg, *ba;     /* [n_kf][3] (in/out) */
    int n_pts;
    double *pts;               /* [n_pts][3] world points (in/out) */
    const float *pt_track_depth;   /* [n_pts] MapPoint::mTrackDepth (bClose = < 10 m, :3284) */
    int n_mono;
    const int32_t *mono_pt, *mono_kf, *mono_cam;   /* [n_mono] */
    const double *mono_obs;    /* [n_mono][2] keypoint (u, v) */
    const float *mono_inv_sigma2;  /* [n_mono] information = I * invSigma2 / uncertainty2 */
    int n_imu;                 /* inertial edges; each also carries one EdgeGyroRW and one EdgeAccRW */
    const int32_t *imu_kf1, *imu_kf2;
    const float *preint;       /* [n_imu][OMV_PREINT_FLOATS] */
    const uint8_t *imu_robust; /* Huber sqrt(16.92) on this inertial edge (last one / bRecInit) */
    const float *imu_info_scale;   /* 1, or 1e-2 on the last edge of the window (:2986) */
    /* EdgeStereo (include/G2oTypes.h:364-402, src/G2oTypes.cc:402-431): left-camera (cam 0)
     * observations with mvuRight >= 0 (Optimizer.cc:3108-3143): obs (u, v, u_R), information
     * I3 * invSigma2, Huber sqrt(7.815); u_R predicted as u - bf / z (ImuCamPose::ProjectStereo,
     * G2oTypes.cc:198-205).  n_stereo = 0 when there is no depth / right coordinate. */
    int n_stereo;
    const int32_t *stereo_pt, *stereo_kf;   /* [n_stereo] */
    const double *stereo_obs;  /* [n_stereo][3] (kpUn.pt.x, kpUn.pt.y, mvuRight); mvuRight >= 0 */
    const float *stereo_inv_sigma2;   /* [n_stereo] */
    float bf;                  /* KeyFrame::mbf (ImuCamPose::bf) */
    /* GeometricCamera type per camera: OMV_CAM_KB8 (cam = KannalaBrandt8 fx fy cx cy k1..k4) or
     * OMV_CAM_PINHOLE (cam = Pinhole fx fy cx cy, the rest ignored: Pinhole::project / projectJac,
     * src/CameraModels/Pinhole.cpp:18-24, :55-65).  NULL: every camera KannalaBrandt8. */
    const int32_t *cam_model;  /* [n_cams] */
} omv_lba_problem;

typedef struct omv_lba_opts {
    int opt_it;            /* 10, or 4 when bLarge */
    double lambda_init;    /* setUserLambdaInit: 1e0, or 1e-2 when bLarge */
    int max_trials;        /* maxTrialsAfterFailure (10) */
    int large;             /* bLarge: disables the FAIL guard */
} omv_lba_opts;

typedef struct omv_lba_result {
    float err, err_end;    /* activeRobustChi2 before / after optimize(), as floats like the reference */
    int status;            /* OMV_LBA_OK / OMV_LBA_FAIL */
    int iterations;        /* LM iterations run (solve() calls) */
    int trials;            /* LM trials (linear solves) in total */
    double lambda;         /* final lambda */
    double *mono_chi2;     /* optional [n_mono]: e->chi2() after optimize (may be NULL) */
    uint8_t *mono_outlier; /* optional [n_mono]: the :3282-3296 outlier test (may be NULL) */
    double *stereo_chi2;   /* optional [n_stereo] */
    uint8_t *stereo_outlier;   /* optional [n_stereo]: chi2 > 7.815 (:3299-3311) */
} omv_lba_result;

typedef struct omv_lba omv_lba;

/* Workspace for problems up to the given sizes (max_mono bounds the visual edges a handle holds:
 * EdgeMono + EdgeStereo; with sharding, the rank's share). */
omv_status omv_lba_create(int max_kf, int max_cams, int max_pts, int max_mono, int max_imu, omv_lba **out);
omv_status omv_lba_destroy(omv_lba *h);
/* Upload a problem (host arrays); the structure (point -> keyframe slots, reduced-system layout,
 * block fill pattern) is analysed on the host once here.  A failed call: OMV_ERR_ARG leaves the handle's
 * previous problem intact, OMV_ERR_HIP leaves it with none; without a problem omv_lba_optimize, _evaluate,
 * _evaluate_stereo, _reset and _debug_solve return OMV_ERR_ARG before any launch. */
omv_status omv_lba_set_problem(omv_lba *h, const omv_lba_problem *p);
/* Run the optimisation on the uploaded problem; on return the state arrays of `p` (Rwb, twb, Rcw,
 * tcw, vel, bg, ba, pts) hold the optimised state and `r` the outcome.  Synchronous. */
omv_status omv_lba_optimize(omv_lba *h, const omv_lba_opts *o, omv_lba_problem *p, omv_lba_result *r);
/* Residual/Jacobian evaluation at the uploaded state for parity: mono_err [n_mono][2],
 * mono_jx [n_mono][6] (2x3), mono_jp [n_mono][12] (2x6), imu_err [n_imu][9] (any may be NULL). */
omv_status omv_lba_evaluate(omv_lba *h, double *mono_err, double *mono_jx, double *mono_jp, double *imu_err);
/* The same for the EdgeStereo edges: err [n_stereo][3], jx [n_stereo][9] (3x3), jp [n_stereo][18] (3x6). */
omv_status omv_lba_evaluate_stereo(omv_lba *h, double *stereo_err, double *stereo_jx, double *stereo_jp);
/* Restore the state uploaded by the last set_problem (device-side copy; for re-runs and benchmarks). */
omv_status omv_lba_reset(omv_lba *h);
/* Per-stage device time of the last optimize: 0 linearise+build, 1 Schur, 2 reduced solve,
 * 3 back-substitution+update+errors; plus the number of trials.  On one rank the stages are timed only
 * with omv_lba_enable_timing(h, 1) (direct launches with events instead of the captured LM step). */
omv_status omv_lba_stage_ms(omv_lba *h, double *ms4, int *trials);
omv_status omv_lba_enable_timing(omv_lba *h, int on);
/* LM driver: 0 (default) keeps g2o's accept / reject / lambda / stop logic on the device (on one rank the steps
 * are captured hipGraphs of four; a sharded solve launches the same gated steps directly, its collectives called
 * in stream order), one control read-back per batch of steps; 1 runs it on the host with a read-back per trial.
 * Both make the same decisions (tests/test_lba_gpu.py). */
omv_status omv_lba_set_driver(omv_lba *h, int host_driven);
/* Host waits (stream synchronisations) of the last omv_lba_optimize's LM loop and its trial count: the device
 * driver waits once per batch of steps, never per trial. */
omv_status omv_lba_host_syncs(omv_lba *h, int *host_syncs, int *trials);

/* Landmark sharding across ranks: two exchanges per LM step, no host wait per step.
 * Call before omv_lba_set_problem.  Every rank then passes the SAME full problem; the handle keeps
 * the rank's contiguous share of the landmarks (in its landmark order) with their edges, and rank 0
 * alone evaluates the inertial / random-walk edges, adds lambda to the pose diagonal and the pose
 * part of computeScale.  Per trial the handle calls
 *     allreduce(ctx, buf, count, stream)   — in-place SUM of `count` doubles of device memory,
 * once on the partial Schur system [packed blocks | b | coef] and once on [chi2 of the current state (when
 * recomputed), chi2 of the trial, scale] (and once on optimize()'s initial chi2).  The call must be enqueued on
 * (or ordered after) `stream`;
 * it returns 0 on success.  ncclAllReduce(buf, buf, count, ncclFloat64, ncclSum, comm, stream)
 * is exactly that.  Every rank solves the identical reduced system; after omv_lba_optimize each
 * rank has written its own landmarks / edges (chi2, outlier) and all keyframes; err / err_end are
 * global.  world == 1 (the default) is the single-GPU path with no calls. */
typedef int (*omv_allreduce_fn)(void *ctx, double *buf, size_t count, void *stream);
omv_status omv_lba_set_comm(omv_lba *h, int rank, int world, omv_allreduce_fn allreduce, void *ctx);
/* Landmarks / visual edges this rank owns after set_problem, and (optional, [n_pts]) the caller
 * indices of its landmarks.  Any pointer may be NULL. */
omv_status omv_lba_shard(omv_lba *h, int32_t *n_pts, int32_t *n_mono, int32_t *pt_index);

/* ------------------------------------------------------------------------------------------------
 * ORBmatcher::SearchForTriangulation(KeyFrame*, KeyFrame*, vector<pair<size_t,size_t>>&, bOnlyStereo,
 * bCoarse) (src/ORBmatcher.cc:1131-1456) for multi-camera keyframes, with pCamera1->epipolarConstrain
 * dispatched on camera 1's type (:1380-1387): KannalaBrandt8::epipolarConstrain / TriangulateMatches /
 * unproject / Triangulate (src/CameraModels/KannalaBrandt8.cpp:219-229, 319-395, 96-126, 414-429;
 * Eigen::JacobiSVD<Matrix4f> restated; pCamera2's unprojectEig / project by its own type) or
 * Pinhole::epipolarConstrain (src/CameraModels/Pinhole.cpp:103-132: F12 = K1^-T [t12]x R12 K2^-1).  One workgroup per keyframe pair; pairs are independent (vbMatched2 is never set).
 * ---------------------------------------------------------------------------------------------- */
#define OMV_TRI_PAIRS 10   /* LL, LR, RL, RR, L-SL, SL-L, SL-SL, R-SR, SR-R, SR-SR (ORBmatcher.cc:1300-1392) */

/* A keyframe in the reference's concatenated keypoint order [L | R | SL | SR] (device pointers). */
typedef struct omv_kf_view {
    int n;                              /* KeyFrame::N */
    int n_left, n_right, n_sideleft;    /* NLeft, NRight, NSideLeft: camera of idx by range (0..3) */
    const omv_kp *kps;                  /* [n] mvKeys / mvKeysRight / mvKeysSideLeft / mvKeysSideRight by idx */
    const uint8_t *desc;                /* [n][32] mDescriptors */
    const uint8_t *has_mp;              /* [n] GetMapPoint(idx) != NULL */
    int n_nodes;                        /* DBoW2::FeatureVector: node ids ascending, CSR of keypoint indices */
    const uint32_t *node_id;            /* [n_nodes] */
    const int32_t *node_start;          /* [n_nodes + 1] */
    const int32_t *node_idx;
    float level_sigma2[16];             /* mvLevelSigma2 (host values) */
} omv_kf_view;

typedef struct omv_tri_pair {
    omv_kf_view kf1, kf2;
    /* R12 (row-major 3x3) | t12 of the camera pairs in OMV_TRI_PAIRS order: T1w * Tw2 composed with the
     * rig (Tll = T1w Tw2, Tlr = T1w Twr2, Trl = Tr1w Tw2, ...: ORBmatcher.cc:1157-1195). */
    float T[OMV_TRI_PAIRS][12];
    int32_t *match12;                   /* device [kf1.n]: vMatches12 (-1 = none); vMatchedPairs = (i, match12[i] >= 0) */
} omv_tri_pair;

/* cams: host [4][8] parameters of the rig's L, R, SL, SR cameras (both keyframes share the rig):
 * KannalaBrandt8 fx fy cx cy k1..k4 or Pinhole fx fy cx cy; cam_model: host [4] OMV_CAM_KB8 /
 * OMV_CAM_PINHOLE per camera, NULL = all KannalaBrandt8.  n_matches: device [n_pairs] (the return value).  The camera-pair transform of a pair of
 * cameras the reference does not list ((L,SR), (SR,L), (R,SL), (SL,R), (SL,SR), (SR,SL)) is whatever the
 * previous candidate of the scan assigned (the reference's R12/t12/pCamera1/pCamera2 persist across
 * iterations); before any assignment it is LL (the reference's R12/t12 are uninitialised there). */
/* Parity hook: KannalaBrandt8::unproject of kp1 (cams2[0]) and kp2 (cams2[1]), JacobiSVD<Matrix4f> V of
 * svd_in (row-major 4x4), TriangulateMatches(kp1, kp2, R12, t12, sigma, unc) on one device thread:
 * out31 = ray1[3] ray2[3] V[16] z p3D[3] x3D[3] uv1[2] (x3D / uv1: the triangulated point and its
 * projection into camera 1 even when a later check rejects it).  Host pointers; synchronous. */
omv_status omv_tri_debug(const float *cams2, const omv_kp *kp1, const omv_kp *kp2, const float *R12, const float *t12,
                         const float *svd_in, float sigma, float unc, float *out31);

omv_status omv_matcher_search_for_triangulation(omv_matcher *m, int n_pairs, const omv_tri_pair *pairs,
                                                const float *cams, const int32_t *cam_model, int only_stereo,
                                                int coarse, int check_ori, int32_t *n_matches, void *stream);

/* ------------------------------------------------------------------------------------------------
 * ORBmatcher::SearchByBoW — Hamming matching of the keypoints that share a vocabulary node (DBoW2
 * FeatureVector, node ids ascending), with the rotation-consistency filter (ComputeThreeMaxima):
 *   OMV_BOW_KF_FRAME  SearchByBoW(KeyFrame *pKF, Frame &F, vpMapPointMatches) (src/ORBmatcher.cc:349-666):
 *                     per keyframe keypoint with a map point, the best unmatched frame keypoint of each
 *                     camera block (L [0, Nleft), R, SL, SR by the frame's ranges; F.n_left = -1: one block),
 *                     left accepted at <= TH_LOW with the nnratio test, right / side blocks accepted at
 *                     <= TH_LOW (their ratio test is `|| true`) and only when the left best passed TH_LOW.
 *                     Called by Tracking::TrackReferenceKeyFrame / Relocalization.
 *   OMV_BOW_KF_KF     SearchByBoW(KeyFrame *pKF1, KeyFrame *pKF2, vpMatches12) (:1006-1129): per pKF1
 *                     keypoint with a map point the best unclaimed pKF2 keypoint with a map point (vbMatched2),
 *                     accepted at < TH_LOW with the nnratio test.  Called by LoopClosing's place recognition.
 * One wavefront per job; jobs are independent.  `kf.has_mp` / `other.has_mp` = GetMapPoint(idx) && !isBad().
 * ---------------------------------------------------------------------------------------------- */
enum { OMV_BOW_KF_FRAME = 0, OMV_BOW_KF_KF = 1 };

typedef struct omv_bow_job {
    omv_kf_view kf;         /* pKF / pKF1 (its kps give the keyframe keypoint angles, mvKeysUn order) */
    omv_kf_view other;      /* F (n_sideleft = -1: no side cameras) / pKF2 */
    int32_t *match;         /* device: OMV_BOW_KF_FRAME [other.n] vpMapPointMatches as the keyframe keypoint
                               index whose map point the frame keypoint received (-1 none);
                               OMV_BOW_KF_KF [kf.n] vpMatches12 as the pKF2 keypoint index (-1 none) */
} omv_bow_job;

/* jobs: host [n_jobs]; n_matches: device [n_jobs] (the reference's return value).  Up to 16384 keypoints
 * per view (OMV_ERR_CAPACITY beyond). */
omv_status omv_matcher_search_by_bow(omv_matcher *m, int n_jobs, const omv_bow_job *jobs, int mode, float nnratio,
                                     int check_ori, int32_t *n_matches, void *stream);
/* Diagnostic: the number of keyframe keypoints whose short candidate list ran out during the sequential walk
 * (the node was rescanned under the current claims), summed over every SearchByBoW call of the process. */
omv_status omv_matcher_bow_rescans(int64_t *total, int reset);

/* ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (src/ORBmatcher.cc:
 * 895-1004): for every level-0 keypoint of F1 in order, Frame::GetFeaturesInArea(vbPrevMatched[i1], windowSize,
 * 0, 0) on F2's grid (the last omv_matcher_assign_grid batch, camera block 0: F2.mvKeysUn), the best candidate
 * whose previous match (vMatchedDistance) is strictly worse, accepted at <= TH_LOW with the nnratio test; a
 * better later F1 keypoint takes the F2 keypoint over; rotation-consistency filter; vbPrevMatched updated to the
 * matched F2 keypoints.  pairs: host [n_pairs][2] (F1, F2) frame indices of the batch; prev_matched: device
 * [n_pairs][kp_cap][2] in/out; matches12: device [n_pairs][kp_cap] (vnMatches12, -1 none); n_matches: device
 * [n_pairs].  F1's keypoints are frame pairs[i][0]'s block 0 (mvKeysUn). */
omv_status omv_matcher_search_for_initialization(omv_matcher *m, int n_pairs, const int32_t *pairs,
                                                 const omv_frame_geom *geom, const omv_kp *kps, const uint8_t *desc,
                                                 const int *n_kp, float *prev_matched, int window, float nnratio,
                                                 int check_ori, int32_t *matches12, int32_t *n_matches, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Pose-inertial optimisation of tracked frames — replaces Optimizer::PoseInertialOptimizationLastKeyFrame
 * (src/Optimizer.cc:5021-5578): Gauss-Newton (4 rounds x 10 iterations, dense LDLT) over the frame's
 * VertexPose / VertexVelocity / VertexGyroBias / VertexAccBias with the last keyframe's vertices fixed;
 * EdgeMonoOnlyPose (G2oTypes.h:330-362, G2oTypes.cc:382-400) and EdgeStereoOnlyPose (:404-431,
 * :433-456) per matched keypoint, one EdgeInertial + EdgeGyroRW + EdgeAccRW; the outlier
 * classification between rounds (chi2 thresholds 12 / 7.5 / 5.991 / 5.991, stereo 15.6 / 9.8 / 7.815 /
 * 7.815, robust kernels dropped after round 3), the "recover not too bad points" pass, and the
 * marginal Hessian the reference stores in Frame::mpcpi.  A batch of frames runs in one launch
 * (one workgroup per frame).
 * ---------------------------------------------------------------------------------------------- */
typedef struct omv_pose_batch {
    int n_frames;
    /* rig (as omv_lba_problem): per camera KannalaBrandt8 parameters and body <-> camera */
    int n_cams;
    const float *cam;                   /* host [n_cams][8] */
    const double *Rcb, *tcb, *Rbc, *tbc;   /* host [n_cams][9] / [3] */
    float bf;                           /* Frame::mbf (EdgeStereoOnlyPose) */
    /* device: frame state (in/out) — ImuCamPose(Frame*) (G2oTypes.cc:74-133) */
    double *Rwb, *twb;                  /* [F][9], [F][3] */
    double *Rcw, *tcw;                  /* [F][n_cams][9], [F][n_cams][3] initial camera poses, updated */
    double *vel, *bg, *ba;              /* [F][3] */
    /* device: Frame::mpLastKeyFrame's vertices (fixed) */
    const double *kf_Rwb, *kf_twb, *kf_vel, *kf_bg, *kf_ba;
    const float *preint;                /* [F][OMV_PREINT_FLOATS] Frame::mpImuPreintegrated */
    /* device: visual edges, frame-major (edges of frame f: [start[f], start[f+1])) */
    const int32_t *mono_start;          /* [F+1] */
    const int32_t *mono_cam, *mono_kp;  /* camera index, keypoint index i of the frame (mvbOutlier[i]) */
    const double *mono_obs;             /* [E][2] */
    const float *mono_inv_sigma2;       /* [E] mvInvLevelSigma2[octave] / uncertainty2 */
    const float *mono_xw;               /* [E][3] MapPoint::GetWorldPos() */
    const uint8_t *mono_close;          /* [E] MapPoint::mTrackDepth < 10 (bClose) */
    const int32_t *stereo_start;        /* [F+1] (all zero: no stereo edges) */
    const int32_t *stereo_cam, *stereo_kp;
    const double *stereo_obs;           /* [S][3] (u, v, mvuRight) */
    const float *stereo_inv_sigma2, *stereo_xw;
    int kp_cap;                         /* per-frame stride of kp_outlier */
    int n_mono, n_stereo;               /* edge totals of the batch (mono_start[F], stereo_start[F]) */
    const int32_t *cam_model;           /* host [n_cams] OMV_CAM_KB8 / OMV_CAM_PINHOLE (as omv_lba_problem); NULL: KB8 */
} omv_pose_batch;

typedef struct omv_pose omv_pose;
omv_status omv_pose_create(int max_frames, int max_edges, omv_pose **out);
omv_status omv_pose_destroy(omv_pose *h);
/* PoseInertialOptimizationLastKeyFrame on every frame of the batch.  kp_outlier (device
 * [F][kp_cap], Frame::mvbOutlier of the keypoints that carry an edge; others untouched), n_good
 * (device [F], the return value nInitialCorrespondences - nBad), H (device [F][225] or NULL, the
 * 15x15 Hessian of ConstraintPoseImu: pose 0-5, v 6-8, bg 9-11, ba 12-14).  Asynchronous. */
omv_status omv_pose_inertial_last_kf(omv_pose *h, const omv_pose_batch *b, int rec_init, uint8_t *kp_outlier,
                                     int32_t *n_good, double *H, void *stream);

/* Optimizer::PoseInertialOptimizationLastFrame (src/Optimizer.cc:5580-6170): as above, but the previous
 * frame's four vertices are free (ids 4-7; the batch's kf_* fields hold Frame::mpPrevFrame's state and
 * `preint` is Frame::mpImuPreintegratedFrame), one EdgeInertial over all six vertex blocks, EdgeGyroRW /
 * EdgeAccRW between the two frames' biases with information from Frame::mpImuPreintegrated's C (the
 * last keyframe's preintegration, :5960-5971), and an EdgePriorPoseImu (G2oTypes.cc:748-785, Huber 5)
 * on the previous frame from its ConstraintPoseImu (pFp->mpcpi).  The mono chi2 threshold is 5.991 in all
 * four rounds (:5992).  H receives the frame's 15x15 block after Optimizer::Marginalize(H, 0, 14)
 * (:3388-3455, pseudo-inverse below 1e-6) — the matrix handed to the ConstraintPoseImu ctor (:6158-6164);
 * run omv_pose_constraint on it to obtain the stored prior.  The previous frame's state is not written
 * back (the reference discards it). */
typedef struct omv_pose_prior {
    const double *Rwb, *twb, *vel, *bg, *ba;   /* device [F][9] / [F][3]: ConstraintPoseImu Rwb, twb, vwb, bg, ba */
    const double *H;                           /* device [F][225]: ConstraintPoseImu::H (after its ctor) */
    const float *preint_kf;                    /* device [F][OMV_PREINT_FLOATS]: Frame::mpImuPreintegrated */
} omv_pose_prior;
omv_status omv_pose_inertial_last_frame(omv_pose *h, const omv_pose_batch *b, const omv_pose_prior *prior,
                                        int rec_init, uint8_t *kp_outlier, int32_t *n_good, double *H, void *stream);

/* Optimizer::PoseOptimization (src/Optimizer.cc:855-1278), the visual-only pose optimisation Tracking runs before the
 * IMU is initialised (Tracking.cc:2924) and in the visual-only configurations: one VertexSE3Expmap (SE3Quat Tcw of
 * camera 0, oplus = exp(dx) * T, se3quat.h:223-257), one unary edge per edge of the batch — mono edges
 * EdgeSE3ProjectXYZOnlyPose (camera 0) / ...ToBody / ...SLPoseToBody / ...SRPoseToBody (camera c through T_c0,
 * OptimizableTypes.cpp:30-171; Huber sqrt(5.991)), stereo edges EdgeStereoSE3ProjectXYZOnlyPose (camera 0 with
 * fx fy cx cy = cam[0][0..3] and bf, types_six_dof_expmap.cpp:339-404; Huber sqrt(7.815)) — and
 * Levenberg-Marquardt (optimization_algorithm_levenberg.cpp:61-169, tau 1e-5, 10 trials) with a dense LDLT: 4 rounds of
 * optimize(10), each from the initial pose, chi2 5.991 / 7.815 outlier classification between rounds, robust kernels
 * dropped after round 3, a single round below 10 edges.  Uses of `b`: n_frames, n_cams, cam, cam_model, bf, the
 * mono_* / stereo_* edge arrays (mono_close unused; stereo_cam ignored: camera 0), kp_cap, n_mono, n_stereo — the
 * inertial state / preintegration fields are ignored.  Edges follow the reference's creation rule: one edge per
 * keypoint (the conventional branch makes a keypoint with mvuRight >= 0 a stereo edge INSTEAD of a mono one).
 *   rig_q / rig_t   host [n_cams][4] (x y z w) / [3]: T_c0 = mTrl / mTsll / mTsrl as SE3Quat (entry 0 unused)
 *   pose_q / pose_t device [F][4] / [F][3] in/out: Frame::GetPose() as the SE3Quat the reference builds (:871-873);
 *                   out: the optimised estimate (unchanged below 3 edges)
 *   kp_outlier      device [F][kp_cap]: mvbOutlier of the edges' keypoints
 *   n_good          device [F]: the return value (nInitialCorrespondences - nBad; 0 below 3 edges)
 * One workgroup per frame; asynchronous. */
omv_status omv_pose_optimization(omv_pose *h, const omv_pose_batch *b, const double *rig_q, const double *rig_t,
                                 double *pose_q, double *pose_t, uint8_t *kp_outlier, int32_t *n_good, void *stream);

/* Kernel choice of the two calls above.  OMV_POSE_AUTO (default): up to 16 frames per call run on the grouped
 * kernel — one frame over `parts` workgroups (0: one per 126 (LastFrame) / 190 (LastKeyFrame) visual edges of the batch's
 * mean frame, at least ceil(edges of the whole batch / 1022) so that no frame's part can overflow, at most 48) that
 * exchange their normal-equation sums every Gauss-Newton iteration, the latency path of Tracking's one-frame call —
 * and larger batches (or a batch whose edges need more than 48 parts) on one workgroup per frame.  OMV_POSE_BATCH / OMV_POSE_GROUPED force one of them (GROUPED needs kp_cap <= 16384).
 * The grouped kernel reports a frame it could not run (more than 1024 visual edges in one workgroup's keypoint
 * range) with n_good = -1 and OMV_ERR_CAPACITY in omv_pose_last_error. */
#define OMV_POSE_AUTO 0
#define OMV_POSE_BATCH 1
#define OMV_POSE_GROUPED 2
omv_status omv_pose_set_mode(omv_pose *h, int mode, int parts);
/* Device error word of the calls since the last read (0, or OMV_ERR_CAPACITY / OMV_ERR_HIP from the grouped kernel);
 * resets it and synchronises `stream`. */
omv_status omv_pose_last_error(omv_pose *h, int32_t *err, void *stream);

/* The pose graph's visual edges of ONE frame from its map-point assignment, on the device — the edge-creation loop
 * of PoseInertialOptimizationLastKeyFrame / LastFrame (src/Optimizer.cc:5079-5330, :5640-5800) for the multi-camera
 * frame (bRight), so SearchByProjection's output feeds the optimisation without a host round trip: per keypoint slot
 * s = cam * kp_cap + i (the [L | R | SL | SR] order) with kp_to_mp[s] >= 0 an EdgeMonoOnlyPose of block cam (obs =
 * keypoint, invSigma2 = inv_level_sigma2[octave] (uncertainty2 = 1 for KannalaBrandt8 / Pinhole), Xw =
 * mp_pos[kp_to_mp[s]], bClose = mp_track_depth < 10), and with uright[s] > 0 also an EdgeStereoOnlyPose of that
 * block; both lists in slot order, counts in mono_start[1] / stereo_start[1] (start[0] = 0) — the omv_pose_batch edge
 * arrays of a one-frame batch (pass max_edges as its n_mono / n_stereo bound; the batch's kp_cap = n_cams * kp_cap).
 * kps / n_kp / kp_to_mp / mp_* / uright: device (uright [n_cams][kp_cap], omv_frame_uright's layout, or NULL = no
 * stereo edges); inv_level_sigma2: host [n_levels].  More than max_edges edges of a kind
 * raise OMV_ERR_CAPACITY in omv_pose_last_error.  Asynchronous. */
omv_status omv_pose_edges_from_matches(omv_pose *h, int n_cams, int kp_cap, const omv_kp *kps, const int *n_kp,
                                       const int32_t *kp_to_mp, const float *mp_pos, const float *mp_track_depth,
                                       const float *inv_level_sigma2, int n_levels, const float *uright, int max_edges,
                                       int32_t *mono_start, int32_t *mono_cam, int32_t *mono_kp, double *mono_obs,
                                       float *mono_inv_sigma2, float *mono_xw, uint8_t *mono_close, int32_t *stereo_start,
                                       int32_t *stereo_cam, int32_t *stereo_kp, double *stereo_obs,
                                       float *stereo_inv_sigma2, float *stereo_xw, void *stream);

/* ConstraintPoseImu ctor (include/G2oTypes.h:639-659) on n matrices: H <- (H + H) / 2 (= H), then its
 * symmetric eigen-decomposition with eigenvalues below 1e-12 zeroed, recomposed.  Device [n][225]
 * (H_out may alias H_in).  Asynchronous. */
omv_status omv_pose_constraint(int n, const double *H_in, double *H_out, void *stream);

/* ---- IMU preintegration ----
 * IMU::Preintegrated::IntegrateNewMeasurement (src/ImuTypes.cc:160-239) over n independent records, as
 * Tracking::PreintegrateIMU drives it (src/Tracking.cc:1675-1712).  Record r integrates the measurements
 * meas[start[r] .. start[r+1]) in order, each (ax ay az wx wy wz dt) with the interpolation of
 * PreintegrateIMU already applied, starting from its current state:
 *   preint  device [n][OMV_PREINT_FLOATS] in/out (dR dV dP JRg JVg JVa JPg JPa b dT C; Initialize() =
 *           identity dR, zeros elsewhere, b = the bias)
 *   avg     device [n][6] in/out avgA | avgW, or NULL
 *   start   device [n+1]; meas device [start[n]][7]
 *   Nga / NgaWalk  host [6]: the diagonals of IMU::Calib::Cov / CovWalk (Eigen::DiagonalMatrix<float, 6>,
 *                  include/ImuTypes.h:126; Tracking.cc:601 builds them from Ng*sf, Na*sf, Ngw/sf, Naw/sf). */
omv_status omv_imu_preintegrate(int n, float *preint, float *avg, const float *meas, const int32_t *start,
                                const float *Nga, const float *NgaWalk, void *stream);

/* ---- DBoW2 vocabulary transform ----
 * TemplatedVocabulary<FORB::TDescriptor, FORB>::transform(features, BowVector&, FeatureVector&, levelsup)
 * (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1194, per feature :1217-1259) as Frame::ComputeBoW /
 * KeyFrame::ComputeBoW call it (src/KeyFrame.cc:207-214, levelsup 4), over a batch of descriptor sets.
 * The vocabulary tree is flattened in loadFromTextFile's node order (node 0 = root, :1338-1424). */
typedef struct omv_vocab {
    int n_nodes, n_words;
    int L;                         /* m_L (FeatureVector level = L - levelsup)                        */
    int scoring;                   /* DBoW2::ScoringType: 0 L1, 1 L2, 2 chi-square, 3 KL, 4 Bhattacharyya, 5 dot product */
    int weighting;                 /* DBoW2::WeightingType: 0 TF_IDF, 1 TF, 2 IDF, 3 BINARY            */
    const int32_t *child_start;    /* device [n_nodes + 1]: m_nodes[i].children as a CSR, file order  */
    const int32_t *child_ids;      /* device [child_start[n_nodes]]                                   */
    const uint8_t *desc;           /* device [n_nodes][32] node descriptors                           */
    const int32_t *word_id;        /* device [n_nodes] m_nodes[i].word_id (leaves)                    */
    const double *weight;          /* device [n_nodes] m_nodes[i].weight (idf; 0 = stopped word)      */
} omv_vocab;

/* n_sets sets of desc [set][cap][32] with n_desc[set] <= cap <= 16384 rows (mDescriptors row order).
 * Per feature (device [set][cap]): word, wval (the word's weight), node (FeatureVector node, -1 if the
 * descent ended above that level).  BowVector (device [set][cap]): bow_word ascending, bow_value, count in
 * bow_n [set].  FeatureVector (device): fv_node [set][cap] ascending, fv_start [set][cap + 1] (offsets
 * into fv_idx [set][cap]), count in fv_n [set].  Stopped words (weight <= 0) are left out of both, as in
 * the reference.  Asynchronous. */
omv_status omv_bow_transform(const omv_vocab *voc, int n_sets, const uint8_t *desc, int cap, const int *n_desc,
                             int levelsup, int32_t *word, double *wval, int32_t *node, int32_t *bow_word,
                             double *bow_value, int32_t *bow_n, int32_t *fv_node, int32_t *fv_start, int32_t *fv_idx,
                             int32_t *fv_n, void *stream);

/* ---- Frame construction tail (src/Frame.cc:1913-1939) ---- */

/* cv::fisheye::undistortPoints parameters of one camera block (GetDepthFromUndistortedPoints,
 * src/Frame.cc:1659-1734): origK / newK as float (fx, fy, cx, cy; the reference's cv::Mat_<float>),
 * dist_coeff as double (k1..k4). */
typedef struct omv_fisheye_undist {
    float K[4];
    double D[4];
    float newK[4];
} omv_fisheye_undist;

/* GetDepthFromUndistortedPoints for every keypoint of every camera block:
 * cv::fisheye::undistortPoints(kp.pt, origK, D, noArray(), newK) (OpenCV >= 4.5 semantics: at most
 * 10 Newton steps, eps 1e-8, theta clipped to pi/2, (-1e6, -1e6) for a flipped / unconverged theta),
 * then d = depth[cam](round(y), round(x)) (0 outside the image) and
 * u_right = kp.x - bf / d where 0 < d <= 20, else -1 (:1736-1763); the reference's mvuRight.
 * The first n_blocks (<= n_cams, <= 8) camera blocks of each frame are processed.
 *   kps / n_kp   device [frame][n_cams][kp_cap] / [frame][n_cams]
 *   depth        device float [frame][n_blocks][depth_h][depth_w] (the undistorted depth images)
 *   undist       host [n_blocks]: the block's parameters (the reference maps L, R, SL, SR to its
 *                cam_id 1, 0, 4, 3, :1916-1922)
 *   u_right      device float [frame][n_blocks][kp_cap]
 *   undist_xy    device float [frame][n_blocks][kp_cap][2] (the undistorted points) or NULL */
omv_status omv_frame_uright(int n_frames, int n_cams, int n_blocks, int kp_cap, const omv_kp *kps, const int *n_kp,
                            const float *depth, int depth_w, int depth_h, const omv_fisheye_undist *undist, float bf,
                            float *u_right, float *undist_xy, void *stream);

/* The cv::vconcat of Frame's per-camera keypoints / descriptors / mvuRight into the dense frame
 * arrays (mDescriptors = [L; R; SL; SR], :1936-1939; mvKeys order of the N-indexed vectors):
 * frame f's keypoints of its first n_blocks (<= n_cams) blocks land at rows [offset[f], offset[f] + N_f),
 * N_f = sum of n_kp[f][0..n_blocks).  uright_in: [frame][n_blocks][kp_cap] (omv_frame_uright's layout).
 *   offset       device int [n_frames + 1] (output; exclusive prefix of N_f, offset[n_frames] = total)
 *   kps_out / desc_out / uright_out   device [total] rows (uright_in / uright_out may be NULL) */
omv_status omv_frame_pack(int n_frames, int n_cams, int n_blocks, int kp_cap, const omv_kp *kps, const uint8_t *desc,
                          const float *uright_in, const int *n_kp, int *offset, omv_kp *kps_out, uint8_t *desc_out,
                          float *uright_out, void *stream);


/* ---- map-point refresh (LocalMapping.cc:338-339, :776-778, :897-898; MapPoint.cc:377) ----------------------------
 * MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:405-490) for a batch of map points: point p's descriptors are
 * rows desc_row[desc_start[p] .. desc_start[p+1]) of `desc` ([rows][32] u8) -- its observations' L / R / SL / SR rows
 * in the reference's mObservations (std::map) order, bad keyframes left out by the caller.  best_row[p] = the row of
 * the descriptor with the least median Hamming distance to the others (vDists[0.5 (N - 1)] of its sorted row, the
 * first on ties), -1 when the point has none (mDescriptor untouched); desc_out[p] (may be NULL) = that descriptor.
 * All pointers device. */
omv_status omv_mappoint_distinctive_descriptors(int n_points, const int32_t *desc_start, const int32_t *desc_row,
                                                const uint8_t *desc, int32_t *best_row, uint8_t *desc_out, void *stream);
/* MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:503-588): per point its observation entries
 * obs_start[p] .. obs_start[p+1] with the entry camera centre obs_center[e] (float3: GetCameraCenter /
 * GetRightCameraCenter / GetSideLeftCameraCenter / GetSideRightCameraCenter of the keyframe, every entry -- the
 * reference does not skip bad keyframes here), its mWorldPos pos[p], the reference keyframe's camera centre
 * ref_center[p], mvScaleFactors[level] of the point's keypoint in it (ref_level_scale[p]) and
 * mvScaleFactors[nLevels - 1] (ref_max_scale[p]).  Out: mNormalVector, mfMinDistance, mfMaxDistance (float, the
 * reference's arithmetic order); a point without entries is left untouched.  All pointers device. */
omv_status omv_mappoint_normal_depth(int n_points, const int32_t *obs_start, const float *obs_center, const float *pos,
                                     const float *ref_center, const float *ref_level_scale, const float *ref_max_scale,
                                     float *normal, float *min_dist, float *max_dist, void *stream);


/* ---- LocalMapping::SearchInNeighbors' fuse sequence (src/LocalMapping.cc:837-889) ------------------------------------
 * The reference runs ORBmatcher::Fuse (ORBmatcher.cc:1458-1647) as a chain of calls that mutate the map between (and
 * within) calls: phase A fuses the current keyframe's map points (ONE snapshot of GetMapPointMatches(), :839) into every
 * target keyframe, camera block by camera block (:840-853); phase B fuses the target keyframes' map points (collected
 * AFTER phase A, non-bad, first occurrence, :859-881) into the current keyframe (:883-889).  Each accepted match either
 * AddObservation + AddMapPoint's, or Replace's the weaker of the two points (MapPoint.cc:316-380: observations moved,
 * the loser bad, the survivor's descriptor recomputed by ComputeDistinctiveDescriptors, :405-483).  A later point's
 * decision reads that state: isBad(), IsInKeyFrame(pKF), GetMapPoint(bestIdx), Observations() and -- through the
 * window search -- GetDescriptor().
 * Here the window searches of every (job, point) are evaluated on the device speculatively (one omv_matcher_search_kf
 * launch per phase), the decisions are walked in the reference's order on the host against the flattened graph, and an
 * entry whose point's descriptor changed since its evaluation (a Replace survivor) is re-evaluated on the device with
 * the recomputed descriptor before it is used (the recomputation itself on the device: the distinctive-descriptor
 * kernel over the observation rows the reference's ComputeDistinctiveDescriptors reads at that moment).  The result is
 * the reference's graph after phase B, plus the ordered edit log a caller replays with the reference's own methods.
 * Phase C (:891-900: ComputeDistinctiveDescriptors / UpdateNormalAndDepth of the current keyframe's points) is
 * omv_mappoint_* on the caller's side.
 * Keyframes are the n_kf frames of the matcher's last omv_matcher_assign_grid batch (C = geom->n_cams <= 4 camera blocks,
 * N-index = block offset + index in the block, NLeft / NRight / NSideLeft = n_kp[kf][0..2]), NUMBERED IN THE ORDER OF
 * THE MAP POINTS' std::map<KeyFrame*, ...> KEYS (observations are kept sorted by keyframe index). */
typedef struct omv_fuse_graph {
    /* keyframes (host) */
    int n_kf;
    const int32_t *n_blocks;            /* [n_kf] camera blocks Fuse runs on: 1 (NLeft == -1), 2, or 4 (side cameras) */
    const omv_se3f *Tcw;                /* [n_kf][C] GetPose / GetRightPose / GetSideLeftPose / GetSideRightPose */
    const float *Ow;                    /* [n_kf][C][3] the matching camera centres */
    const float *uright;                /* [n_kf][kp_cap] mvuRight of block 0 (host; AddObservation's nObs += 2 when
                                           the keyframe has one camera), or NULL */
    int32_t *kf_mps;                    /* [n_kf][C * kp_cap] in/out: mvpMapPoints by N-index (entries [0, N) of each
                                           keyframe's row): map-point index or -1 */
    /* map points (host): the snapshot of the points the keyframes reference */
    int n_mps;
    int32_t *bad;                       /* [n_mps] in/out isBad() */
    int32_t *n_obs;                     /* [n_mps] in/out Observations() (nObs) */
    int32_t *replaced;                  /* [n_mps] out: the point it was Replace'd by, or -1 */
    const int32_t *obs_start;           /* [n_mps + 1] in: mObservations rows, keyframe order */
    const int32_t *obs_kf;              /* [rows] keyframe index */
    const int32_t *obs_idx;             /* [rows][4] left / right / side-left / side-right N-index or -1 */
    /* out: the final mObservations (CSR with capacity), the edit log */
    int32_t *out_obs_start;             /* [n_mps + 1] */
    int32_t *out_obs_kf;                /* [obs_cap] */
    int32_t *out_obs_idx;               /* [obs_cap][4] */
    int obs_cap;
    int32_t *log;                       /* [log_cap][4]: {0, mp, kf, idx} AddObservation(pKF, idx) + pKF->AddMapPoint;
                                           {1, a, b, -1} a->Replace(b); in the reference's order */
    int log_cap;
    int32_t n_log;                      /* out: entries written (OMV_ERR_CAPACITY past log_cap / obs_cap) */
    int32_t n_reevaluated;              /* out: entries re-evaluated after a descriptor change (diagnostic) */
    int32_t n_device_calls;             /* out: device round trips (diagnostic) */
} omv_fuse_graph;

/* current: the current keyframe's index; targets: host [n_targets] vpTargetKFs in order; mps: the device map-point
 * table (pos / normal / min_dist / max_dist as GetWorldPos / GetNormal / mfMinDistance / mfMaxDistance; desc is
 * UPDATED IN PLACE to the final descriptors); p: omv_kf_search_params with mode OMV_KF_FUSE, th 3, max_dist TH_LOW
 * (50); geom / kps / desc / n_kp: the assign_grid batch (device).  n_fused: host [n_targets * C + C] per Fuse call,
 * phase A (target-major, block-minor) then phase B; calls the reference does not make (blocks past n_blocks) are 0.
 * Synchronous. */
omv_status omv_search_in_neighbors_fuse(omv_matcher *m, const omv_frame_geom *geom, const omv_kp *kps,
                                        const uint8_t *desc, const int *n_kp, int kp_cap, omv_fuse_graph *g,
                                        int current, int n_targets, const int32_t *targets, const omv_kf_mps *mps,
                                        const omv_kf_search_params *p, int32_t *n_fused, void *stream);

/* ---- LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:395-783) ---------------------------------------------------
 * The reference walks the current keyframe's neighbours in order (:439).  Per neighbour pKF2: the baseline test
 * (:447-461: |Ow2 - Ow1| < pKF2->mb skips it when !mbMonocular; Ow1 is the PERSISTENT side-1 camera centre, see below),
 * SearchForTriangulation(mpCurrentKeyFrame, pKF2) (:468), and for every match (idx1, match12[idx1]) in idx1 order the
 * camera-pair state (listed pairs (0,0) (0,1) (1,0) (1,1) when both rigs have a second camera, (0,2) (2,0) (2,2) (1,3)
 * (3,1) (3,3) when they have four, :529-636; other pairs keep the previous match's state), parallax of the unprojected
 * rays, GeometricTools::Triangulate (JacobiSVD<Matrix4f>) or KeyFrame::UnprojectStereo, positive depth, reprojection
 * error in both keyframes, scale consistency; an accepted match creates a MapPoint and mpCurrentKeyFrame->AddMapPoint(
 * pMP, idx1) (:766-781) -- so every LATER neighbour's SearchForTriangulation skips idx1 (ORBmatcher.cc:1223-1227).
 * The state that crosses matches and neighbours: sophTcw1 / Ow1 (side 1's camera block, declared before the loop,
 * :419-424) persists across neighbours; pCamera1 / pCamera2 and side 2 reset per neighbour (:445, :470-474).  Float
 * arithmetic as the reference (no contraction; glibc atan2f / cosf / tanf restated).  Creating the MapPoint objects and
 * the graph updates (AddObservation, pKF2->AddMapPoint, ComputeDistinctiveDescriptors, UpdateNormalAndDepth) stay with
 * the caller (the last two: omv_mappoint_*); the current keyframe's has-map-point flags are updated here. */
typedef struct omv_cnmp_kf {
    omv_kf_view kf;                     /* kps by idx (mvKeysUn when NLeft == -1, else mvKeys / Right / SideLeft /
                                           SideRight by range), n_left = -1 for a single-camera keyframe, level_sigma2;
                                           desc / has_mp / nodes: read by omv_local_mapping_create_new_map_points'
                                           SearchForTriangulation (neighbours; the current keyframe's has_mp is the
                                           separate in/out array), unused by omv_create_new_map_points */
    const omv_kp *kps_raw;              /* [n] mvKeys for KeyFrame::UnprojectStereo (NULL: kf.kps) */
    float Tcw[4][12];                   /* GetPose / GetRightPose / GetSideLeftPose / GetSideRightPose: Rcw (row-major) | tcw */
    float Ow[4][3];                     /* GetCameraCenter / GetRightCameraCenter / GetSideLeft.. / GetSideRight.. */
    float Rwc[9], twc[3];               /* mRwc, mTwc.translation() (UnprojectStereo) */
    float fx, fy, cx, cy, invfx, invfy; /* the keyframe's fx fy cx cy invfx invfy */
    float mb, mbf;                      /* mb: also the neighbour's baseline threshold (:453) */
    const float *uright, *depth;        /* device [n] mvuRight / mvDepth (NULL: no stereo observations) */
    float scale_factors[16];            /* mvScaleFactors */
} omv_cnmp_kf;

typedef struct omv_cnmp_job {
    omv_cnmp_kf kf2;                    /* the neighbour */
    const int32_t *match12;             /* device [kf1.kf.n]: SearchForTriangulation's vMatches12 (-1 none; entries
                                           outside [0, kf2.kf.n) are ignored) */
    float *x3D;                         /* device [kf1.kf.n][3]: the new point of an accepted match */
    int32_t *status;                    /* device [kf1.kf.n]: 1 triangulated, 2 by UnprojectStereo (bPointStereo),
                                           0 rejected, no match, or the neighbour skipped by the baseline test */
} omv_cnmp_job;

/* The per-match geometry of CreateNewMapPoints for jobs whose match lists the caller obtained itself (e.g. the
 * single-camera stereo rigs SearchForTriangulation's device path does not cover).  Jobs run in order with the
 * reference's state chain: check_baseline = !mbMonocular (the baseline test against the persistent Ow1);
 * side1_state: device int32 in/out, side 1's camera block (sophTcw1 / Ow1) entering the first job and leaving the last
 * (0 = the current keyframe's left camera, the value at the top of CreateNewMapPoints; NULL: 0, not returned);
 * has_mp1: device [kf1.kf.n] or NULL, set to 1 at every accepted idx1 (:773).
 * EXACTNESS: a job's match12 must be the SearchForTriangulation result computed AFTER the previous jobs' AddMapPoint
 * (has_mp1), as the reference computes it per neighbour (:468).  A caller-driven loop passes one job per call
 * (SearchForTriangulation with kf1.has_mp = has_mp1, then this call with the same side1_state); several jobs in one
 * call are exact only when no accepted idx1 of an earlier job appears in a later job's list.
 * omv_local_mapping_create_new_map_points runs the whole loop on the device.
 * cams / cam_model: host [4][8] / [4] (the rig's L, R, SL, SR; NULL model = all KannalaBrandt8; others OMV_ERR_ARG);
 * n_cams: cameras of the rig (1: mpCamera2 == NULL, 2: L + R, 4: L R SL SR); inertial: mbInertial; far_points /
 * th_far_points: mbFarPoints / mThFarPoints; scale_factor: the current keyframe's mfScaleFactor (ratioFactor =
 * 1.5 scale_factor).  jobs: host array (n_jobs <= 64).  Asynchronous. */
omv_status omv_create_new_map_points(int n_jobs, const omv_cnmp_kf *kf1, const omv_cnmp_job *jobs, const float *cams,
                                     const int32_t *cam_model, int n_cams, int inertial, int far_points,
                                     float th_far_points, float scale_factor, int check_baseline,
                                     int32_t *side1_state, uint8_t *has_mp1, void *stream);

/* One neighbour of omv_local_mapping_create_new_map_points. */
typedef struct omv_cnmp_neighbour {
    omv_cnmp_kf kf2;                    /* kf2.kf: the full view SearchForTriangulation reads (kps, desc, has_mp =
                                           pKF2->GetMapPoint(idx2) != NULL, FeatureVector, level_sigma2) */
    float T[OMV_TRI_PAIRS][12];         /* the camera-pair transforms, as omv_tri_pair.T (keyframe 1 = current) */
    int skip;                           /* the caller's `continue` before the search: mbMonocular's median-depth
                                           ratio test (:455-461); the stereo baseline test is done here */
    int32_t *match12;                   /* device [kf1.kf.n] out: the neighbour's vMatches12 (all -1 when skipped) */
    float *x3D;                         /* device [kf1.kf.n][3] out, as omv_cnmp_job */
    int32_t *status;                    /* device [kf1.kf.n] out, as omv_cnmp_job */
} omv_cnmp_neighbour;

/* LocalMapping::CreateNewMapPoints' loop (:439-783) for a multi-camera rig (n_cams 2 or 4: the rigs
 * omv_matcher_search_for_triangulation covers), on the device with no host round trip between neighbours: per
 * neighbour in order, the baseline gate on the persistent Ow1, SearchForTriangulation(mpCurrentKeyFrame, pKF2,
 * bOnlyStereo = false, bCoarse = coarse) with the matcher's checkOri off (ORBmatcher matcher(0.6, false), :417) against
 * the current keyframe's has-map-point flags AS LEFT BY THE PREVIOUS NEIGHBOURS, then the per-match geometry, then
 * AddMapPoint(idx1) of the accepted matches.
 *   kf1        the current keyframe (kf1.kf: kps, desc, FeatureVector, level_sigma2, ranges; kf1.kf.has_mp ignored)
 *   has_mp1    device [kf1.kf.n] in/out: GetMapPoint(idx1) != NULL on entry, plus every accepted idx1 on return
 *   nb         host [n_nb] (n_nb <= 64) neighbours in vpNeighKFs order
 *   n_matches  device [n_nb]: SearchForTriangulation's return values (0 for a skipped neighbour)
 *   side1_state device int32 in/out or NULL (as omv_create_new_map_points): calls compose, so a caller that checks
 *              CheckNewKeyFrames() between neighbours (:440) runs one neighbour per call with the same has_mp1 /
 *              side1_state and gets the identical result
 * check_baseline = !mbMonocular; the other arguments as omv_create_new_map_points.  Synchronises `stream` once at the
 * end (the device error word: OMV_ERR_CAPACITY for a keyframe past SearchForTriangulation's limits). */
omv_status omv_local_mapping_create_new_map_points(omv_matcher *m, const omv_cnmp_kf *kf1, uint8_t *has_mp1, int n_nb,
                                                   const omv_cnmp_neighbour *nb, const float *cams,
                                                   const int32_t *cam_model, int n_cams, int inertial,
                                                   int check_baseline, int coarse, int far_points, float th_far_points,
                                                   float scale_factor, int32_t *n_matches, int32_t *side1_state,
                                                   void *stream);

/* ------------------------------------------------------------------------------------------------
 * Sim3Solver (src/Sim3Solver.cc, include/Sim3Solver.h): the Horn RANSAC of LoopClosing::DetectCommonRegionsFromBoW
 * (src/LoopClosing.cc:812-832), between SearchByBoW and SearchByProjection / SearchBySim3.  One handle holds n_jobs
 * independent solvers (one per candidate pair); the phases are the reference's: constructor + SetRansacParameters
 * (omv_sim3_solver_set), iterate / find (omv_sim3_solver_iterate), the GetEstimated* accessors (omv_sim3_solver_best).
 * Arithmetic: float in the reference's order except ComputeSim3's eigenvector step (a Jacobi in double in place of
 * Eigen::EigenSolver<Matrix4f> + atan2 + SO3f::exp: the same rotation, not the same bits).
 * ---------------------------------------------------------------------------------------------- */
#define OMV_SIM3_NO_MORE 1    /* flags bit 0: bNoMore   */
#define OMV_SIM3_CONVERGE 2   /* flags bit 1: bConverge */
typedef struct omv_sim3_solver omv_sim3_solver;

/* max_jobs solvers, max_corr_total correspondences over all of them, max_hyp hypotheses per omv_sim3_solver_iterate. */
omv_status omv_sim3_solver_create(int max_jobs, int max_corr_total, int max_hyp, omv_sim3_solver **out);
omv_status omv_sim3_solver_destroy(omv_sim3_solver *h);

/* The constructor's numeric part (:119-179) and SetRansacParameters(prob, min_inliers[j], max_its) (:184-207) for every
 * job; resets the carried state (mnIterations = 0, mnBestInliers = 0).  Every pointer is HOST memory.  Job j owns the
 * correspondences corr_start[j] .. corr_start[j+1]-1 (corr_start[0] = 0), in the order the constructor pushes them:
 *   Xw1, Xw2    [n][3] pMP1 / pMP2->GetWorldPos()            sigma2_1, sigma2_2  [n] mvLevelSigma2[kp.octave] per side
 *   index1      [n] mvnIndices1 (i1 in vpMatched12), each < mN1[j] = vpMatched12.size()
 *   pose1/2     [n_jobs][12] Riw row-major then tiw: pKF->GetRotation / GetTranslation(cameraID)
 *   cam1/2      [n_jobs][8] fx fy cx cy k0..k3, model1/2 [n_jobs] OMV_CAM_KB8 / OMV_CAM_PINHOLE, fix_scale [n_jobs]
 * The thresholds keep the reference's quirk: mvnMaxError1/2 are std::vector<size_t>, so 9.210 * sigma2 is truncated to
 * an unsigned integer.  ransac_max_its_out [n_jobs] (or NULL) receives mRansacMaxIts.  A job with fewer
 * correspondences than min_inliers (iterate's entry test), or fewer than three (the reference is undefined there), is
 * born with bNoMore and does no work.  OMV_ERR_ARG: an unknown camera model, a negative size, an index1 outside
 * [0, mN1); OMV_ERR_CAPACITY: more jobs / correspondences than the handle's.  Synchronises `stream`. */
omv_status omv_sim3_solver_set(omv_sim3_solver *h, int n_jobs, const int32_t *corr_start, const float *Xw1,
                               const float *Xw2, const float *sigma2_1, const float *sigma2_2, const int32_t *index1,
                               const int32_t *mN1, const float *pose1, const float *pose2, const float *cam1,
                               const float *cam2, const int32_t *model1, const int32_t *model2, const int32_t *fix_scale,
                               double prob, const int32_t *min_inliers, int max_its, int32_t *ransac_max_its_out,
                               void *stream);

/* iterate(nIterations, bNoMore, vbInliers, nInliers, bConverge) (:273-346) for every job, asynchronous on `stream`;
 * every pointer is DEVICE memory.  draws [n_jobs][n_iterations][3]: for hypothesis k of the call the three values
 * DUtils::Random::RandomInt(0, size-1) returns, draw i in [0, N-1-i] (out-of-range values are clamped).  A job runs
 * min(n_iterations, mRansacMaxIts - mnIterations) hypotheses, stops at the first one the reference returns from, and
 * is skipped once it has converged or is exhausted (its outputs are repeated).  Draws after a convergence are unused:
 * a caller that mirrors rand() draws them all the same, so its rand() sequence runs ahead of the reference's.
 *   T12_out [n_jobs][16] row-major: mBestT12 (the converged hypothesis, else the best so far -- the reference's
 *           5-argument iterate returns an uninitialised matrix when no hypothesis of the chunk reached the carried best;
 *           identity before any hypothesis).  The 4-argument iterate / find return identity unless bConverge.
 *   n_inliers_out [n_jobs]; inliers_out: vbInliers, job j's mN1[j] bytes at sum(mN1[0..j-1]);
 *   flags_out [n_jobs]: OMV_SIM3_NO_MORE | OMV_SIM3_CONVERGE.  n_iterations <= max_hyp (OMV_ERR_CAPACITY). */
omv_status omv_sim3_solver_iterate(omv_sim3_solver *h, int n_iterations, const int32_t *draws, float *T12_out,
                                   int32_t *n_inliers_out, uint8_t *inliers_out, int32_t *flags_out, void *stream);

/* GetEstimatedRotation / Translation / Scale of job `job` (mBestRotation row-major, mBestTranslation, mBestScale), with
 * mnBestInliers and mnIterations; host outputs, any may be NULL.  Synchronises `stream`. */
omv_status omv_sim3_solver_best(omv_sim3_solver *h, int job, float *R, float *t, float *scale, int32_t *n_best,
                                int32_t *iterations, void *stream);

/* Test hook: the hypotheses job `job` evaluated in the last omv_sim3_solver_iterate call, host outputs (any but n_hyp
 * may be NULL): n_hyp = H, idx [H][3] the sampled correspondences, R [H][9], t [H][3], scale [H], T12 / T21 [H][16],
 * count [H] mnInliersi, mask_words [H][ceil(N / 64)] mvbInliersi (bit i of word i / 64).  Synchronous. */
omv_status omv_sim3_solver_debug(omv_sim3_solver *h, int job, int32_t *n_hyp, int32_t *idx, float *R, float *t,
                                 float *scale, float *T12, float *T21, int32_t *count, uint64_t *mask_words,
                                 void *stream);

/* ------------------------------------------------------------------------------------------------
 * MLPnPsolver (src/MLPnPsolver.cpp, include/MLPnPsolver.h): the PnP RANSAC of Tracking::Relocalization
 * (src/Tracking.cc:3543-3730), between SearchByBoW and PoseOptimization.  One handle holds n_jobs independent solvers
 * (one per candidate keyframe of a frame; many frames may share a handle); the phases are the reference's: constructor
 * + SetRansacParameters (omv_pnp_set), iterate (omv_pnp_iterate).
 * Arithmetic: computePose in double as the reference's, CheckInliers in its mixed double / float.  Not bit-exact: the
 * JacobiSVDs are cyclic Jacobi eigen-decompositions, sums run in correspondence order per matrix entry, mlpnpJacs is the
 * same derivative through the chain rule, the eigenvectors of the planarity matrix have a fixed sign.  Refine keeps
 * computePose's result for its CheckInliers, and its outcome is kept with the carried state (a pure function of
 * mvbBestInliers).
 * ---------------------------------------------------------------------------------------------- */
#define OMV_PNP_NO_MORE 1   /* flags bit 0: bNoMore                    */
#define OMV_PNP_FOUND 2     /* flags bit 1: iterate's return value     */
typedef struct omv_pnp omv_pnp;

/* max_jobs solvers, max_corr_total correspondences over all of them, max_hyp hypotheses per omv_pnp_iterate. */
omv_status omv_pnp_create(int max_jobs, int max_corr_total, int max_hyp, omv_pnp **out);
omv_status omv_pnp_destroy(omv_pnp *h);

/* The constructor's numeric part (:28-45) and SetRansacParameters(prob, min_inliers, max_its, min_set, epsilon, th2)
 * (:177-218) for every job; resets the carried state (mnIterations = 0, mnBestInliers = 0).  Every pointer is HOST
 * memory.  Job j owns the correspondences corr_start[j] .. corr_start[j+1]-1 (corr_start[0] = 0), in the order the
 * constructor pushes them:
 *   P2D    [n][2] F.mvKeysUn[i].pt        sigma2 [n] F.mvLevelSigma2[kp.octave]        Xw [n][3] pMP->GetWorldPos()
 *   index  [n] mvKeyPointIndices (i in vpMapPointMatches), each < mN[j] = vpMapPointMatches.size()
 *   cam    [n_jobs][8] fx fy cx cy k0..k3, model [n_jobs] OMV_CAM_KB8 / OMV_CAM_PINHOLE
 * The header's defaults are (0.99, 8, 300, 6, 0.4, 5.991); Tracking passes (0.99, 10, 300, 6, 0.5, 5.991).
 * ransac_max_its_out / ransac_min_inliers_out [n_jobs] (or NULL) receive mRansacMaxIts / mRansacMinInliers.  A job with
 * fewer correspondences than mRansacMinInliers (iterate's entry test) does no work and reports bNoMore.
 * OMV_ERR_ARG: min_set != 6, an unknown camera model, a negative size, an index outside [0, mN); OMV_ERR_CAPACITY: more
 * jobs / correspondences than the handle's.  Synchronises `stream`. */
omv_status omv_pnp_set(omv_pnp *h, int n_jobs, const int32_t *corr_start, const float *P2D, const float *sigma2,
                       const float *Xw, const int32_t *index, const int32_t *mN, const float *cam, const int32_t *model,
                       double prob, int min_inliers, int max_its, int min_set, float epsilon, float th2,
                       int32_t *ransac_max_its_out, int32_t *ransac_min_inliers_out, void *stream);

/* iterate(nIterations, bNoMore, vbInliers, nInliers, Tout) (:56-175) for every job, asynchronous on `stream`; every
 * pointer is DEVICE memory.  The reference's loop condition is an OR (:75): a call runs
 * max(n_iterations, mRansacMaxIts - mnIterations) hypotheses unless it returns earlier -- the whole RANSAC on the first
 * call, n_iterations more on every later one.  draws [n_jobs][n_draws][6]: for hypothesis k of the call the six values
 * DUtils::Random::RandomInt(0, size-1) returns, draw i in [0, N-1-i] (out-of-range values are clamped); a job runs at
 * most n_draws hypotheses, so n_draws >= max(n_iterations, mRansacMaxIts) gives the reference's call.  Draws after a
 * return are unused.
 *   T_out [n_jobs][16] row-major: mRefinedTcw when Refine succeeded, mBestTcw at exhaustion, else identity
 *   n_inliers_out [n_jobs]; inliers_out: vbInliers, job j's mN[j] bytes at sum(mN[0..j-1]);
 *   flags_out [n_jobs]: OMV_PNP_NO_MORE | OMV_PNP_FOUND.  n_draws <= max_hyp (OMV_ERR_CAPACITY). */
omv_status omv_pnp_iterate(omv_pnp *h, int n_iterations, int n_draws, const int32_t *draws, float *T_out,
                           int32_t *n_inliers_out, uint8_t *inliers_out, int32_t *flags_out, void *stream);

/* Test hook: what job `job` did in the last omv_pnp_iterate call, host outputs (any but n_hyp / n_refine may be NULL).
 * n_hyp = H hypotheses up to the one the call returned at:
 *   hyp_int  [H][10]  the six sampled correspondences, planar flag, Gauss-Newton iterations, exit reason (0 five
 *                     iterations, 1 max|Jac dx| < 1e-5, 2 the 5.0 / 1.0 break, 3 no finite step), mnInliersi
 *   hyp_pose [H][24]  doubles: the linear stage R0 [9], t0 [3], the final R [9], t [3]
 *   mask_words [H][ceil(N / 64)] mvbInliersi (bit i of word i / 64)
 * n_refine = K Refine calls, in order:
 *   ref_int  [K][8]   the hypothesis that became best, its inlier count, planar, iterations, exit reason,
 *                     mnRefinedInliers, success, 0
 *   ref_pose [K][24], ref_mask_words [K][ceil(N / 64)] as above for the refined pose
 * state_out [6]: mnIterations, mnBestInliers, a Refine outcome is kept, its count, its success, what the call returned
 * (0 identity, 1 the refined outcome, 2 the best).  prepared [N][12]: per correspondence the bearing, its two nullspace
 * vectors and Xw, in double.  Synchronous. */
omv_status omv_pnp_debug(omv_pnp *h, int job, int32_t *n_hyp, int32_t *hyp_int, double *hyp_pose, uint64_t *mask_words,
                         int32_t *n_refine, int32_t *ref_int, double *ref_pose, uint64_t *ref_mask_words,
                         int32_t *state_out, double *prepared, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Optimizer::OptimizeSim3 (src/Optimizer.cc:2460-2726): the Sim3 refinement of LoopClosing's loop / merge candidates
 * (src/LoopClosing.cc:658, :899, :935), after Sim3Solver and between the SearchByProjection calls.  One call optimises
 * n_jobs independent candidate pairs, one wavefront each.  Double arithmetic as g2o's, except that the two projection
 * edges are differentiated analytically where g2o differentiates them numerically (delta 1e-9): the result agrees with
 * the reference's to within that scheme's own noise, not bit for bit.
 * ---------------------------------------------------------------------------------------------- */
#define OMV_OPTSIM3_KEPT 0        /* match kept, not counted: P3D2c.z < 0 (no edge), or the call returned 0 early */
#define OMV_OPTSIM3_INLIER 1      /* counted in n_in                                                             */
#define OMV_OPTSIM3_REMOVED_1 2   /* vpMatches1[i] nulled after the first round                                  */
#define OMV_OPTSIM3_REMOVED_2 3   /* vpMatches1[i] nulled by the final test                                      */
typedef struct omv_optsim3 omv_optsim3;

/* A handle for up to max_jobs candidate pairs and max_entries_total correspondences over all of them per call. */
omv_status omv_optimize_sim3_create(int max_jobs, int max_entries_total, omv_optsim3 **out);
omv_status omv_optimize_sim3_destroy(omv_optsim3 *h);

/* Every pointer is HOST memory; the call synchronises `stream`.  Job j owns the entries entry_start[j] ..
 * entry_start[j+1]-1 (entry_start[0] = 0): the i of vpMatches1 that pass the graph-side tests of :2522-2589 (a match, the
 * keypoint on cameraID1, both map points present and not bad, i2 >= 0 || bAllPoints), in ascending i.  Per entry:
 *   Xw1, Xw2      [n][3] pMP1 / pMP2->GetWorldPos()            obs1 [n][2] kp1.pt, inv_sigma2_1 [n] mvInvLevelSigma2[octave]
 *   has_kp2       [n] i2 >= 0; then obs2 [n][2] = kp2.pt and inv_sigma2_2 [n] its level's; otherwise obs2 is computed
 *                 (pCamera2->project(P3D2c) in float) and inv_sigma2_2 is that of pMP2->GetTrackScaleLevel(cameraID2)
 * Per job: pose1/2 [12] Riw row-major then tiw (GetRotation / GetTranslation(cameraID)), cam1/2 [8] fx fy cx cy k0..k3,
 * model1/2 OMV_CAM_KB8 / OMV_CAM_PINHOLE, fix_scale, th2, and g2oS12 in / out as q [4] (x y z w), t [3], s.
 * Outputs: n_in [n_jobs] the return value; status [n] per entry (OMV_OPTSIM3_*): vpMatches1[i] is nulled for 2 and 3,
 * and n_in is the number of entries with status 1.  The reference's quirks are kept: an entry with P3D2c.z < 0 is no
 * edge and keeps its match; the round-one test reads the edges' stale errors; with fewer than 10 pairs left after round
 * one the call returns 0 with g2oS12 untouched and the round-one removals in place; a NaN chi2 fails every `> th2`
 * test, so its pair is kept and counted.  mAcumHessian is zero in the reference (set, never filled): not an output.
 * OMV_ERR_ARG: an unknown camera model, a negative size or a descending entry_start, more jobs or entries than the
 * handle holds, a NULL pointer with a non-zero size. */
omv_status omv_optimize_sim3(omv_optsim3 *h, int n_jobs, const int32_t *entry_start, const float *Xw1, const float *Xw2,
                             const float *obs1, const float *inv_sigma2_1, const uint8_t *has_kp2, const float *obs2,
                             const float *inv_sigma2_2, const float *pose1, const float *pose2, const float *cam1,
                             const float *cam2, const int32_t *model1, const int32_t *model2, const int32_t *fix_scale,
                             const float *th2, double *q, double *t, double *s, int32_t *n_in, uint8_t *status,
                             void *stream);

/* Test hook: job `job` of the last omv_optimize_sim3 call, host outputs (any may be NULL).  The first buildSystem (at
 * the input estimate, robust): H [49] row-major, b [7], chi2 (activeRobustChi2), lambda_init, x [7] the first trial's
 * solution; e12, e21 [n][2] the residuals of every pair at the input estimate (0 where no edge); per round [2] the LM
 * iterations, the trials, and the largest number of trials in one iteration.  Synchronous. */
omv_status omv_optimize_sim3_debug(omv_optsim3 *h, int job, double *H, double *b, double *chi2, double *lambda_init,
                                   double *x, double *e12, double *e21, int32_t *iterations, int32_t *trials,
                                   int32_t *max_trials, void *stream);

/* ------------------------------------------------------------------------------------------------
 * KeyFrameDatabase (src/KeyFrameDatabase.cc): add / erase / clear / clearMap, DetectNBestCandidates (:581-713, called at
 * src/LoopClosing.cc:562) and DetectRelocalizationCandidates (:715-828, called at src/Tracking.cc:3551) on the device,
 * for a batch of queries, bit-exact.  L1 scoring only (omv_vocab.scoring == 0, what ORBvoc uses): any other `scoring`
 * is OMV_ERR_ARG.
 *
 * The database is a table of BowVectors by slot; the caller chooses a keyframe's slot in [0, max_kf) and keeps the
 * KeyFrame* <-> slot map.  There is no inverted file: lKFsSharingWords is the occupied slots that share a word with the
 * query, in ascending (smallest shared word, sequence number of the slot's latest add), which is the order the
 * reference's walk over mvInvertedFile produces.  Per slot and per mode the handle keeps the reference's persistent
 * pair (mnPlaceRecognitionQuery, mPlaceRecognitionScore) / (mnRelocQuery, mRelocScore); add resets both to (0, 0), a
 * fresh KeyFrame (the reference never initialises mRelocScore; it is 0 here), with no neighbours and flags 0; erase
 * leaves the state in place (a keyframe out of the database is still a neighbour with its stored score).  A keyframe
 * is listed iff it shares a word, is not in the query's connected set (n_best only) and its stored id differs from the
 * query's; listing stores the id.  The neighbour loop adds the STORED score of every neighbour whose stored id is the
 * query's, stale or not.  So a query with id 0 lists no fresh keyframe, and a repeated id lists nothing again.
 * The queries of one call behave exactly as the same queries made one per call, in order.
 *
 * What stays with the caller and arrives as arrays: GetConnectedKeyFrames() of the query, GetBestCovisibilityKeyFrames(10)
 * of the database keyframes, isBad(), the map id and Map::IsBad().  One stream at a time per handle.  add, erase, clear,
 * clear_map, set_neighbours and set_flags synchronise `stream`; the two detect calls do not.
 * ---------------------------------------------------------------------------------------------- */
typedef struct omv_kfdb omv_kfdb;

omv_status omv_kfdb_create(int scoring, int max_kf, int max_bow, int max_queries, int max_query_bow, omv_kfdb **out);
omv_status omv_kfdb_destroy(omv_kfdb *h);

/* KeyFrameDatabase::add for n keyframes.  slot, map_id [n]: host.  bow_word, bow_value [n][stride], bow_n [n]: device,
 * as omv_bow_transform leaves them (word ids ascending).  Sequence numbers follow call order, then array order.
 * OMV_ERR_ARG: a slot out of range, occupied or named twice, bow_n outside [0, stride]; OMV_ERR_CAPACITY: bow_n >
 * max_bow.  Nothing is changed on an error. */
omv_status omv_kfdb_add(omv_kfdb *h, int n, const int32_t *slot, const int32_t *map_id, const int32_t *bow_word,
                        const double *bow_value, const int32_t *bow_n, int stride, void *stream);
/* erase (slot [n] host; erasing an empty slot is a no-op, as in the reference), clear, clearMap. */
omv_status omv_kfdb_erase(omv_kfdb *h, int n, const int32_t *slot, void *stream);
omv_status omv_kfdb_clear(omv_kfdb *h, void *stream);
omv_status omv_kfdb_clear_map(omv_kfdb *h, int map_id, void *stream);
/* GetBestCovisibilityKeyFrames(10) of the named slots: neigh host [n][10] slots in the reference's order, -1 padded (a
 * keyframe that never had a slot is -1).  flags host [n]: bit 0 isBad(), bit 1 GetMap()->IsBad(). */
omv_status omv_kfdb_set_neighbours(omv_kfdb *h, int n, const int32_t *slot, const int32_t *neigh, void *stream);
omv_status omv_kfdb_set_flags(omv_kfdb *h, int n, const int32_t *slot, const uint8_t *flags, void *stream);

/* DetectNBestCandidates for n_q queries, in order.  Host: query_id [n_q] pKF->mnId, query_map [n_q], conn_start
 * [n_q + 1] (conn_start[0] = 0, ascending) and conn_slot: the slots of GetConnectedKeyFrames() that are in the
 * database.  Device: q_bow_word / q_bow_value [n_q][stride], q_bow_n [n_q], and the outputs loop_out / merge_out
 * [n_q][n_candidates] (slots in the reference's order, -1 beyond the count) and n_loop / n_merge [n_q].  A q_bow_n
 * outside [0, min(stride, max_query_bow)] gives that query the counts -1.  Asynchronous. */
omv_status omv_kfdb_detect_n_best(omv_kfdb *h, int n_q, const int64_t *query_id, const int32_t *query_map,
                                  const int32_t *conn_start, const int32_t *conn_slot, const int32_t *q_bow_word,
                                  const double *q_bow_value, const int32_t *q_bow_n, int stride, int n_candidates,
                                  int32_t *loop_out, int32_t *n_loop, int32_t *merge_out, int32_t *n_merge,
                                  void *stream);
/* DetectRelocalizationCandidates: frame_id [n_q] F->mnId and map_id [n_q] host; cand_out device [n_q][max_kf] in
 * lAccScoreAndMatch order, n_cand [n_q].  Asynchronous. */
omv_status omv_kfdb_detect_reloc(omv_kfdb *h, int n_q, const int64_t *frame_id, const int32_t *map_id,
                                 const int32_t *q_bow_word, const double *q_bow_value, const int32_t *q_bow_n,
                                 int stride, int32_t *cand_out, int32_t *n_cand, void *stream);
/* Test hook: query `query` of the last detect call, host outputs, any may be NULL; arrays hold up to max_kf entries.
 * maxCommonWords, minCommonWords (0 when nothing is listed); lKFsSharingWords as list_slot / list_words [n_list];
 * lScoreAndMatch as scored_slot [n_scored] with the double score before the cast and the float si; lAccScoreAndMatch
 * in its final order (sorted for n_best, as built for reloc) as acc_bits (the float's bits) / acc_best [n_scored].
 * Synchronous. */
omv_status omv_kfdb_debug(omv_kfdb *h, int query, int32_t *max_common_words, int32_t *min_common_words,
                          int32_t *n_list, int32_t *list_slot, int32_t *list_words, int32_t *n_scored,
                          int32_t *scored_slot, double *score, float *si, uint32_t *acc_bits, int32_t *acc_best,
                          void *stream);

/* ------------------------------------------------------------------------------------------------
 * Optimizer::InertialOptimization (src/Optimizer.cc:3469-3925): the IMU initialisation of LocalMapping::InitializeIMU
 * (src/LocalMapping.cc:1255-1517), ScaleRefinement (:1548) and LoopClosing (src/LoopClosing.cc:2037), batched over
 * n_jobs independent maps, one workgroup each.  The three overloads are modes:
 *   FULL (:3469-3653)  velocities, bg, ba, gravity direction free, the scale iff mono; Levenberg, optimize(200), lambda
 *                      init 1e3 only if priorG != 0 (otherwise tau * max diagonal); EdgePriorAcc / EdgePriorGyro
 *   BIAS (:3655-3813)  velocities, bg, ba free; Rwg = I and scale = 1 (Rwg / scale are not read and come back
 *                      untouched); Levenberg, optimize(200), lambda init 1e3; the same priors
 *   GS   (:3815-3925)  gravity direction and scale free; Gauss-Newton, optimize(10); Huber (delta 1); no priors
 * ---------------------------------------------------------------------------------------------- */
#define OMV_INERTIAL_FULL 0
#define OMV_INERTIAL_BIAS 1
#define OMV_INERTIAL_GS 2
#define OMV_INERTIAL_MAX_KF 320   /* keyframes of one job (the elimination's working set lives in LDS) */
typedef struct omv_inertial_opt omv_inertial_opt;

/* A handle for up to max_jobs jobs, max_kf_total keyframes and max_edges_total edges over all of them per call. */
omv_status omv_inertial_opt_create(int max_jobs, int max_kf_total, int max_edges_total, omv_inertial_opt **out);
omv_status omv_inertial_opt_destroy(omv_inertial_opt *h);

/* Every pointer is HOST memory; the call synchronises `stream`.  Job j owns the keyframes kf_start[j] .. kf_start[j+1]-1
 * and the edges edge_start[j] .. edge_start[j+1]-1 (both start at 0).  Per keyframe (the vertices of :3503-3520, i.e.
 * mnId <= maxKFid): Rwb [9] row-major and twb [3], the body pose as VertexPose(KeyFrame*) forms it; vel_in [3];
 * old_gyro_bias [3], GetGyroBias() before the call.  Per edge (the tests of :3571-3594: mPrevKF set, both ids
 * <= maxKFid, the keyframe not bad): edge_kf1 / edge_kf2, the previous and the current keyframe as indices into the
 * job's keyframes, and preint [OMV_PREINT_FLOATS], the current keyframe's record.  Per job: bg0 / ba0 [3], the bias of
 * vpKFs.front() (every bias vertex is built from it; in GS mode the fixed bias of every edge), mode (OMV_INERTIAL_*),
 * mono, priorG, priorA, and Rwg [9] / scale in and out.
 * Outputs: Rwg, scale, bg [3], ba [3] per job; per keyframe vel [3] (double), vel_f32 [3] (what SetVelocity stores) and
 * reintegrate: 1 iff (old_gyro_bias - (float)bg).norm() > 0.01 in float, the records Reintegrate() is called on (GS: 0,
 * and bg, ba, vel are the inputs); iterations / trials per job: solver iterations and linear solves.
 * The edges of a job must form simple paths (mPrevKF is a single link): a keyframe that is kf1 of two edges or kf2 of
 * two, an index outside the job, a cycle are OMV_ERR_ARG; a keyframe without an edge is a legal vertex.  OMV_ERR_ARG also
 * for a negative size or a descending start array, an unknown mode, more than OMV_INERTIAL_MAX_KF keyframes in a job,
 * more jobs / keyframes / edges than the handle holds, a NULL pointer with a non-zero size. */
omv_status omv_inertial_optimization(omv_inertial_opt *h, int n_jobs, const int32_t *kf_start, const int32_t *edge_start,
                                     const double *Rwb, const double *twb, const double *vel_in, const float *old_gyro_bias,
                                     const int32_t *edge_kf1, const int32_t *edge_kf2, const float *preint,
                                     const double *bg0, const double *ba0, const int32_t *mode, const int32_t *mono,
                                     const float *priorG, const float *priorA, double *Rwg, double *scale, double *bg,
                                     double *ba, double *vel, float *vel_f32, uint8_t *reintegrate, int32_t *iterations,
                                     int32_t *trials, void *stream);

/* Test hook: job `job` of the last call, host outputs in the job's own keyframe / edge order (any may be NULL).  e0
 * [E][9] the residuals at the input state.  The first buildSystem: Hvv [K][9] the velocity diagonal blocks, Hvoff [E][9]
 * the V1-rows x V2-columns block of every edge, border [K][3][9] (columns bg ba gdir(2) scale), bv [K][3], corner [81],
 * bc [9], chi2 (activeRobustChi2), lambda_init; rows and columns of fixed unknowns are zero.  xv [K][3], xc [9]: the
 * first trial's solution.  iterations, trials, max_trials (the most trials of one iteration); err [2]: GS mode's float
 * robust chi2 before and after; ticks [3]: the workgroup's time in buildSystem, in the linear solves and in the trials'
 * error evaluations, in ticks of the device's constant 100 MHz clock.  Synchronous. */
omv_status omv_inertial_opt_debug(omv_inertial_opt *h, int job, double *e0, double *Hvv, double *Hvoff, double *border,
                                  double *bv, double *corner, double *bc, double *chi2, double *lambda_init, double *xv,
                                  double *xc, int32_t *iterations, int32_t *trials, int32_t *max_trials, float *err,
                                  int64_t *ticks, void *stream);
/* Test hook, host only (no device needed): the path planner on one job.  order [K] position -> keyframe, pos_of [K],
 * edge_in / edge_out [K] per position (-1: none), n_paths.  OMV_ERR_ARG where omv_inertial_optimization rejects. */
omv_status omv_inertial_opt_plan(int K, int E, const int32_t *kf1, const int32_t *kf2, int32_t *order, int32_t *pos_of,
                                 int32_t *edge_in, int32_t *edge_out, int32_t *n_paths);

/* ---- Test hooks (no reference counterpart): the device linear-algebra routines on plain device arrays ----
 * Each launches the product's own instantiation of the routine, one workgroup per problem (`batch` problems, on
 * `stream`, not synchronised).  Every pointer is device memory. */

/* The pivoted LDL^T solves of the pose kernels.  routine 0: ldlt_pick_solve<n>, n in {6, 9, 24}; `order` receives the
 * pick order (position -> row).  routine 1: ldlt_pivot_solve_wave<n>, n in {15, 30}; `order` receives the
 * transpositions.  H [batch][n * n] row-major, b [batch][n]; x [batch][n] and order [batch][n] are in / out: the caller
 * pre-fills them, what the routine does not write comes back unchanged; ok [batch]: the routine's result (isPositive). */
omv_status omv_selftest_ldlt(int routine, int n, int batch, const double *H, const double *b, double *x, int32_t *order,
                             int32_t *ok, void *stream);
/* pinv15_wave: A [batch][225] -> P [batch][225]; path [batch]: 1 when the routine's entry predicate (both LDL^T
 * factorisations with positive pivots, evaluated by the hook on the same input) selects the inverse, 0 the Jacobi
 * eigen-decomposition. */
omv_status omv_selftest_pinv15(int batch, const double *A, double *P, int32_t *path, void *stream);
/* inertial_info9_wave<par != 0>: the float covariance C [batch][15 * 15] -> info [batch][81]; path [batch]: 0 the
 * factorisation shortcut (par only: the result is the symmetrised inverse itself, no rotation applied), 1 the
 * eigen-decomposition with every eigenvalue kept, 2 with at least one eigenvalue below 1e-12 zeroed. */
omv_status omv_selftest_inertial_info9(int par, int batch, const float *C, double *info, int32_t *path, void *stream);
/* inv16 of the reduced system's solver (the LDS instantiation): D [batch][256], 16 x 16 blocks in the solver's layout
 * (entry (r, c) at 16 r + (c ^ r)), only the lower triangle read -> Dinv [batch][256], the full inverse in the same
 * layout; bad [batch]: the routine's flag (a zero or non-finite pivot). */
omv_status omv_selftest_inv16(int batch, const double *D, double *Dinv, int32_t *bad, void *stream);

/* The float layer under the bit-exact kernels (csrc/omv_math.h, rcp_nr, the plain `/` and `a * b + c` of the build
 * flags), elementwise over n elements of device memory, one thread per element, on `stream` (not synchronised).
 * float unless noted; [n] unless noted:
 *   SINCOSF a -> out [n][2] (sin, cos)      ATANF, TANF, SQRTF a -> out      ATAN2F, FAST_ATAN2_DEG (a = y, b = x) -> out
 *   ROUND_EVEN a -> int32                   DIVF a / b                       MULADD_F32 a * b + c (plain operators)
 *   MULADD_F64 the same on doubles          RCP_NR double a -> double
 *   KB8_PROJECT / PINHOLE_PROJECT     a = X [n][3], b = k[8] -> uv [n][2]
 *   KB8_UNPROJECT / PINHOLE_UNPROJECT a = px [n][2], b = k[8] -> ray [n][3]
 *   PREDICT_SCALE a = ratio, b[0] = log scale factor -> int32 (int)ceil(log((double)a) / (double)b[0])
 *   PREDICT_SCALE_CLAMPED the same with b[1] = the number of levels (as a float) -> int32 clamped to [0, levels - 1]
 *   ROT_BIN (a = angle1, b = angle2) -> int32, the matchers' rotation-histogram bin
 *   THREE_MAXIMA a = int32 histograms [n][30] -> int32 [n][3], ComputeThreeMaxima's indices (-1: absent)
 *   GRID_CELL_OF a = keypoint (x, y) [n][2], b = (min_x, min_y, cell width inverse, cell height inverse) -> int32, the
 *                grid cell column * 48 + row of Frame::PosInGrid (-1: outside the grid)
 *   GRID_WINDOW  a = (x, y, r) [n][3], b as above -> int32 [n][4], the cells (min column, max column, min row, max
 *                row) Frame::GetFeaturesInArea visits; four -1 when the window misses the grid
 *   KP_IN_WINDOW a = (keypoint x, y, octave, window x, y, r, minLevel, maxLevel) [n][8], the three integers as floats
 *                -> int32 1 / 0, GetFeaturesInArea's test of one keypoint of a visited cell
 * An unknown fn, n < 0, or a NULL among the pointers fn reads with n > 0: OMV_ERR_ARG before any launch; n == 0:
 * OMV_OK. */
#define OMV_MATH_SINCOSF 0
#define OMV_MATH_ATANF 1
#define OMV_MATH_ATAN2F 2
#define OMV_MATH_TANF 3
#define OMV_MATH_SQRTF 4
#define OMV_MATH_FAST_ATAN2_DEG 5
#define OMV_MATH_ROUND_EVEN 6
#define OMV_MATH_DIVF 7
#define OMV_MATH_MULADD_F32 8
#define OMV_MATH_MULADD_F64 9
#define OMV_MATH_RCP_NR 10
#define OMV_MATH_KB8_PROJECT 11
#define OMV_MATH_KB8_UNPROJECT 12
#define OMV_MATH_PINHOLE_PROJECT 13
#define OMV_MATH_PINHOLE_UNPROJECT 14
#define OMV_MATH_PREDICT_SCALE 15
#define OMV_MATH_ROT_BIN 16
#define OMV_MATH_THREE_MAXIMA 17
#define OMV_MATH_PREDICT_SCALE_CLAMPED 18
#define OMV_MATH_GRID_CELL_OF 19
#define OMV_MATH_GRID_WINDOW 20
#define OMV_MATH_KP_IN_WINDOW 21
omv_status omv_selftest_math(int fn, int64_t n, const void *a, const void *b, const void *c, void *out, void *stream);

/* One reduced-system solve on a handle after omv_lba_set_problem, at the current state: errors, build, assemble and
 * the block LDL^T once, through the optimiser's own launches, with the damping `lambda` (> 0: the padding pivots are
 * lambda) and the robust kernels of the problem (`o` is validated only: no option changes them).  Host outputs, n =
 * 16 n_opt: S [n * n] the reduced system scattered dense in keyframe order (row 16 k + r; the stored lower blocks
 * mirrored, padding rows included), rhs [n] = b - the Schur right-hand side, x [n] the solution, fail the solver's
 * flag, plan [plan_cap >= 4 + n_opt]: storage mode (1 every block in LDS, 2 hybrid LDS / global, 0 global), n_slots,
 * n_lds, n_lev, then the columns per level.  Synchronous. */
omv_status omv_lba_debug_solve(omv_lba *h, const omv_lba_opts *o, double lambda, double *S, double *rhs, double *x,
                               int32_t *fail, int32_t *plan, int plan_cap);

/* Test hooks on the library's memory ownership (process-wide).  live_allocations: the device, pinned-host and
 * stream-ordered allocations the library holds now (every handle's buffers and the per-call workspaces).
 * fail_allocation: the nth next allocation of the library (1-based) fails without a HIP call, as if the device were
 * out of memory, and the hook disarms itself; 0 disarms, nth < 0 is OMV_ERR_ARG. */
omv_status omv_debug_live_allocations(int64_t *n);
omv_status omv_debug_fail_allocation(int nth);

/* ------------------------------------------------------------------------------------------------
 * Optimizer::LocalBundleAdjustment (src/Optimizer.cc:1280-1830), and the graph Optimizer::BundleAdjustment (:40-366)
 * and the merge overload of LocalBundleAdjustment (:3927-4363) share: VertexSE3Expmap keyframes, VertexSBAPointXYZ
 * points, EdgeSE3ProjectXYZ / ...ToBody / ...SLToBody / ...SRToBody and g2o::EdgeStereoSE3ProjectXYZ edges,
 * BlockSolver_6_3 with Levenberg.  The visual kind of the omv_lba solver: the same Schur complement, block LDL^T, LM
 * control and host plan; state, Jacobians, update, lambda_0 and outlier test are this graph's.  Single rank.
 * The caller flattens its window (host-side selection and write-back stay with the caller) and keeps the state on the
 * device between calls: optimize(5), set_levels + Huber 0, optimize(10) is the merge overload's two rounds.
 * ---------------------------------------------------------------------------------------------- */
struct omv_vba_problem {
    int n_cams;
    const float *cam;          /* [n_cams][8] fx fy cx cy k1..k4 (Pinhole: fx fy cx cy) */
    const int32_t *cam_model;  /* [n_cams] OMV_CAM_KB8 / OMV_CAM_PINHOLE; NULL: every camera KannalaBrandt8 */
    const double *q_c0, *t_c0; /* [n_cams][4] (x y z w), [n_cams][3]: camera c <- camera 0 (mTrl, mTsll, mTsrl); camera 0
                                  is the vertex's own camera (identity) */
    int n_kf, n_opt;           /* keyframes; the first n_opt optimisable, the rest fixed (the InitKF among them) */
    double *q_cw, *t_cw;       /* [n_kf][4] (x y z w), [n_kf][3]: camera 0's Tcw (in/out) */
    int n_pts;
    double *pts;               /* [n_pts][3] (in/out) */
    int n_mono;                /* 2-row edges: camera 0 -> EdgeSE3ProjectXYZ, camera c > 0 -> the ToBody edge of T_c0[c] */
    const int32_t *mono_pt, *mono_kf, *mono_cam;
    const double *mono_obs;    /* [n_mono][2] */
    const float *mono_inv_sigma2;
    int n_stereo;              /* g2o::EdgeStereoSE3ProjectXYZ on camera 0 */
    const int32_t *stereo_pt, *stereo_kf;
    const double *stereo_obs;  /* [n_stereo][3] (u, v, u_R >= 0) */
    const float *stereo_inv_sigma2;
    double fx, fy, cx, cy, bf; /* the stereo edges' pinhole (pKF->fx ... mbf, floats widened) */
};
typedef struct omv_vba_problem omv_vba_problem;

struct omv_vba_opts {
    int iterations;            /* optimize(n) */
    double lambda_init;        /* setUserLambdaInit (100 on an inertial map); <= 0: computeLambdaInit = 1e-5 max |diag H| */
    int max_trials;            /* maxTrialsAfterFailure (10) */
    double huber_mono, huber_stereo;   /* Huber deltas: (float)sqrt(5.991) / (float)sqrt(7.815); 0 = no robust kernel */
};
typedef struct omv_vba_opts omv_vba_opts;

struct omv_vba_result {
    double err, err_end;       /* activeRobustChi2 before optimize() / of the last computed errors */
    int iterations, trials;
    double lambda;             /* final lambda */
    double lambda_init;        /* the lambda_0 used (computeLambdaInit's when opts.lambda_init <= 0) */
    double *mono_chi2;         /* optional [n_mono]: e->chi2() at the final state (excluded edges too) */
    uint8_t *mono_outlier;     /* optional [n_mono]: chi2 > 5.991 || !isDepthPositive (depth in the edge's camera) */
    double *stereo_chi2;       /* optional [n_stereo] */
    uint8_t *stereo_outlier;   /* optional [n_stereo]: chi2 > 7.815 || !isDepthPositive */
};
typedef struct omv_vba_result omv_vba_result;

typedef struct omv_vba omv_vba;

/* Capacities: keyframes, cameras, points, edges (2-row + stereo).  A problem beyond them is OMV_ERR_CAPACITY. */
omv_status omv_vba_create(int max_kf, int max_cams, int max_pts, int max_edges, omv_vba **out);
omv_status omv_vba_destroy(omv_vba *h);
/* Upload and plan a problem; every edge at level 0.  OMV_ERR_ARG (a NULL or out-of-range field) and OMV_ERR_CAPACITY
 * leave the previous problem as it was, OMV_ERR_HIP leaves none.  Without a problem every call below is OMV_ERR_ARG
 * before any launch. */
omv_status omv_vba_set_problem(omv_vba *h, const omv_vba_problem *p);
/* Edge levels in the caller's order (0 = active, 1 = excluded: it adds nothing to errors, chi2 sums or the system; a
 * point whose edges are all excluded does not move).  NULL arrays: every edge of that kind active. */
omv_status omv_vba_set_levels(omv_vba *h, const uint8_t *mono_level, const uint8_t *stereo_level);
/* optimize(o->iterations) from the state on the device (it stays there for the next call); q_cw, t_cw and pts of `p`
 * receive the new state.  Synchronous. */
omv_status omv_vba_optimize(omv_vba *h, const omv_vba_opts *o, omv_vba_problem *p, omv_vba_result *r);
/* Errors and Jacobians at the device state for parity (any may be NULL): mono_err [n_mono][2], mono_jxi [n_mono][6]
 * (2x3), mono_jxj [n_mono][12] (2x6, (omega, upsilon)); stereo_err [n_stereo][3], jxi [.][9], jxj [.][18]. */
omv_status omv_vba_evaluate(omv_vba *h, const omv_vba_opts *o, double *mono_err, double *mono_jxi, double *mono_jxj,
                            double *stereo_err, double *stereo_jxi, double *stereo_jxj);
/* The state uploaded by the last set_problem again (the levels stay). */
omv_status omv_vba_reset(omv_vba *h);
/* omv_lba_debug_solve for this kind (Huber deltas from `o`); S, rhs, x, plan as there. */
omv_status omv_vba_debug_solve(omv_vba *h, const omv_vba_opts *o, double lambda, double *S, double *rhs, double *x,
                               int32_t *fail, int32_t *plan, int plan_cap);
/* omv_lba_enable_timing / omv_lba_stage_ms for this kind. */
omv_status omv_vba_enable_timing(omv_vba *h, int on);
omv_status omv_vba_stage_ms(omv_vba *h, double *ms4, int *trials);

/* ------------------------------------------------------------------------------------------------
 * Optimizer::FullInertialBA (src/Optimizer.cc:368-853): the whole map's inertial bundle adjustment, as LocalMapping::
 * InitializeIMU runs it after InertialOptimization and Map::ApplyScaledRotation (src/LocalMapping.cc:1387-1406), VIBA 1 /
 * VIBA 2 and the global BA of an inertial map.  The full inertial kind of the omv_lba solver: the same edges (EdgeMono,
 * EdgeStereo, EdgeInertial), Schur complement, block LDL^T, LM control and host plan.  Every EdgeInertial is Huber
 * sqrt(16.92) at its full information (:514-516); there is no outlier round and no FAIL guard.
 *   shared_bias == 0 (bInit false): every bImu keyframe has its own VertexGyroBias / VertexAccBias, and every inertial
 *     edge carries one EdgeGyroRW and one EdgeAccRW (:520-538).
 *   shared_bias == 1 (bInit): all keyframes share one pair, which vertices G and A of every EdgeInertial are; no
 *     random-walk edges; EdgePriorGyro / EdgePriorAcc (error 0 - b, information prior * I3, no robust kernel) on the pair
 *     (:441-450, :484-487, :544-563).  The pair starts at bg0 / ba0 (pIncKF's bias) and every bImu keyframe holds it on
 *     return (:818-829).  The reduced system then has one more block, bordering every keyframe with an inertial edge.
 * base: the flattened map as an omv_lba_problem -- with bFixLocal the maxKFid keyframe is listed last and n_opt = n_kf
 * - 1, otherwise n_opt = n_kf; kf_imu 0: a pose vertex only; inertial edges between two bImu keyframes only (:469);
 * pt_track_depth, imu_robust and imu_info_scale are not read (may be NULL).  A map point seen by fixed keyframes only
 * is no vertex (:771-774): it does not move and its edges add nothing.  Single rank.
 * Left with the caller: SetNewBias(prevKF->GetImuBias()) on every preintegration before the call (:470), the nLoopId
 * != 0 write-back into the *GBA members, pbStopFlag, Map::ApplyScaledRotation, MergeInertialBA.
 * ---------------------------------------------------------------------------------------------- */
struct omv_fiba_problem {
    omv_lba_problem base;      /* rig, keyframes, points, visual and inertial edges (state in/out) */
    int shared_bias;           /* bInit */
    double prior_g, prior_a;   /* priorG / priorA (floats widened to double, :554, :560); >= 0; read when shared_bias */
    double bg0[3], ba0[3];     /* the shared pair's starting value; read when shared_bias */
};
typedef struct omv_fiba_problem omv_fiba_problem;

struct omv_fiba_opts {
    int iterations;            /* its: optimize(its) */
    double lambda_init;        /* setUserLambdaInit(1e-5) (:393) */
    int max_trials;            /* maxTrialsAfterFailure (10) */
};
typedef struct omv_fiba_opts omv_fiba_opts;

struct omv_fiba_result {
    double err, err_end;       /* activeRobustChi2 before optimize() / of the last computed errors */
    int iterations, trials;
    double lambda;             /* final lambda */
    double *mono_chi2;         /* optional [n_mono]: e->chi2() at the final state; 0 on an edge that is not in the graph */
    double *stereo_chi2;       /* optional [n_stereo] */
};
typedef struct omv_fiba_result omv_fiba_result;

typedef struct omv_fiba omv_fiba;

/* Capacities: keyframes, cameras, points, visual edges (EdgeMono + EdgeStereo), inertial edges. */
omv_status omv_fiba_create(int max_kf, int max_cams, int max_pts, int max_edges, int max_imu, omv_fiba **out);
omv_status omv_fiba_destroy(omv_fiba *h);
/* Upload and plan a problem.  OMV_ERR_ARG before any launch, the previous problem kept: a size beyond the capacities
 * (n_kf > max_kf, n_imu > max_imu, ...), an out-of-range index, and with shared_bias no inertial edge, an inertial edge on a keyframe
 * that is not bImu, or a negative or non-finite prior.  OMV_ERR_HIP leaves no problem. */
omv_status omv_fiba_set_problem(omv_fiba *h, const omv_fiba_problem *p);
/* optimize(o->iterations) from the state on the device (it stays there for the next call); the state arrays of
 * p->base receive the result.  Synchronous. */
omv_status omv_fiba_optimize(omv_fiba *h, const omv_fiba_opts *o, omv_fiba_problem *p, omv_fiba_result *r);
/* Errors and visual Jacobians at the device state for parity, in the caller's edge order (any may be NULL; zero on an
 * edge that is not in the graph): as omv_lba_evaluate / omv_lba_evaluate_stereo, then prior_err [6]: EdgePriorGyro's and
 * EdgePriorAcc's errors 0 - b (zero without a shared pair). */
omv_status omv_fiba_evaluate(omv_fiba *h, double *mono_err, double *mono_jx, double *mono_jp, double *imu_err,
                             double *stereo_err, double *stereo_jx, double *stereo_jp, double *prior_err);
/* The state uploaded by the last set_problem again. */
omv_status omv_fiba_reset(omv_fiba *h);
/* omv_lba_debug_solve for this kind; n = 16 (n_opt + shared_bias): the shared pair is block n_opt (rows 9..14, the
 * rest padding); plan_cap >= 4 + n_opt + shared_bias. */
omv_status omv_fiba_debug_solve(omv_fiba *h, double lambda, double *S, double *rhs, double *x, int32_t *fail,
                                int32_t *plan, int plan_cap);
/* omv_lba_enable_timing / omv_lba_stage_ms for this kind. */
omv_status omv_fiba_enable_timing(omv_fiba *h, int on);
omv_status omv_fiba_stage_ms(omv_fiba *h, double *ms4, int *trials);

/* ------------------------------------------------------------------------------------------------
 * Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:1826-2119), its map-merging overload (:2121-2458) and
 * Optimizer::OptimizeEssentialGraph4DoF (:6171-6480): the pose graph over every keyframe of the map that
 * LoopClosing::CorrectLoop and MergeLocal run between the Sim3 alignment and the global BA.  g2o's Levenberg-Marquardt
 * (20 iterations of up to 10 trials) with the edges' numeric Jacobians (base_binary_edge.hpp:131-205), on the block
 * LDL^T of the omv_lba solver.  Single rank.
 *   OMV_ESSGRAPH_SIM3: g2o::VertexSim3Expmap vertices (q x y z w, t, s: 8 doubles), g2o::EdgeSim3 edges, error
 *     log(C S_i S_j^-1) with vertex 0 = i, vertex 1 = j, C = S_table[j] S_table[i]^-1, information I7, lambda_0 = 1e-16;
 *     oplus Sim3(update) * estimate, update[6] = 0 under fix_scale.
 *   OMV_ESSGRAPH_4DOF: VertexPose4DoF vertices ([Rcw 9 | tcw 3 | Rwb 9 | twb 3] row-major: camera 0's pose and the body
 *     pose of ImuCamPose(pKF) or ImuCamPose(Rwc, twc, pKF); 24 doubles), Edge4DoF edges with the rotation and
 *     translation of S_table[i] S_table[j]^-1 (scale dropped), information diag(1e3, 1e3, 1, 1, 1, 1), lambda_0 =
 *     computeLambdaInit; oplus ImuCamPose::UpdateW((0, 0, u0, u1, u2, u3)) with its normalisation of DR after every
 *     fifth kept update.
 * The caller walks the map (GetAllKeyFrames, isBad, parents, loop edges, covisibility, sInsertedEdges, the minFeat
 * test) and hands the graph over flat, the edges in the reference's creation order.  S_a is vScw (the CorrectedSim3
 * entry where there is one, else the pose with scale 1); S_b the NonCorrectedSim3 entry, else vScw.  The merge overload
 * is the same call: its two fixed sets are fixed flags, its vpGoodPose / vpBadPose choice is the per-edge table.
 * Parallel edges between one pair sum; an edge between two fixed vertices adds to chi2 only.
 * ---------------------------------------------------------------------------------------------- */
enum { OMV_ESSGRAPH_SIM3 = 0, OMV_ESSGRAPH_4DOF = 1 };
/* omv_essgraph_recover: which SetPose the poses are for (:2083-2088, :2419-2423, :6443-6450) */
enum { OMV_ESSGRAPH_RECOVER_LOOP = 0, OMV_ESSGRAPH_RECOVER_MERGE = 1, OMV_ESSGRAPH_RECOVER_4DOF = 2 };

struct omv_essgraph_problem {
    int n_vertices;
    const double *vertices;    /* [n_vertices][8] (Sim3 kind) or [n_vertices][24] (4DoF kind): the start values */
    const uint8_t *fixed;      /* [n_vertices] setFixed */
    const double *S_a, *S_b;   /* [n_vertices][8] the two Sim3 tables the measurements are composed from */
    int n_edges;
    const int32_t *edge_i, *edge_j;   /* g2o's vertex 0 / vertex 1 */
    const int32_t *edge_table;        /* 0: S_a, 1: S_b */
    int fix_scale;             /* Sim3 kind: VertexSim3Expmap::_fix_scale of every vertex */
    const double *Rcb, *tcb;   /* 4DoF kind: [9], [3] the rig's mImuCalib.mTcb (camera 0); not read by the Sim3 kind */
};
typedef struct omv_essgraph_problem omv_essgraph_problem;

struct omv_essgraph_result {
    double err, err_end;       /* activeChi2 before optimize() / of the last computed errors */
    int iterations, trials;
    int solver_failed;         /* a linear solve of this optimize() hit a zero or non-finite pivot */
    double lambda;             /* final lambda */
    double *vertices;          /* optional [n_vertices][8 or 24]: the final estimates, layout as the problem's */
};
typedef struct omv_essgraph_result omv_essgraph_result;

typedef struct omv_essgraph omv_essgraph;

/* OMV_ERR_ARG: an unknown kind, max_vertices < 1 or max_edges < 0. */
omv_status omv_essgraph_create(int kind, int max_vertices, int max_edges, omv_essgraph **out);
omv_status omv_essgraph_destroy(omv_essgraph *h);
/* Upload and plan a graph; the measurements are composed on the device.  OMV_ERR_ARG before any launch, the previous
 * problem kept: a null array, a problem beyond the capacities, an edge naming a vertex that is not there, i == j, a
 * table other than 0 / 1, no optimisable vertex.  OMV_ERR_HIP leaves no problem. */
omv_status omv_essgraph_set_problem(omv_essgraph *h, const omv_essgraph_problem *p);
/* optimize(iterations) with maxTrialsAfterFailure = max_trials from the state on the device (it stays there).  The LM
 * control runs on the device: one host wait per call.  Synchronous. */
omv_status omv_essgraph_optimize(omv_essgraph *h, int iterations, int max_trials, omv_essgraph_result *r);
/* At the device state, per edge (any may be NULL): err [n_edges][7 or 6]; jac_i / jac_j [n_edges][7 x 7 or 6 x 4]
 * row-major, g2o's numeric _jacobianOplusXi / Xj (zero for a fixed vertex); meas [n_edges][8] the Sim3 C, or
 * [n_edges][12] Edge4DoF's [dRij 9 | dtij 3]; chi2 [n_edges]. */
omv_status omv_essgraph_evaluate(omv_essgraph *h, double *err, double *jac_i, double *jac_j, double *meas, double *chi2);
/* The state uploaded by the last set_problem again. */
omv_status omv_essgraph_reset(omv_essgraph *h);
/* One linear solve at `lambda` from the device state: the n x n system (n = 16 blocks; optimisable vertices in caller
 * order, two Sim3 vertices per block at rows 0-6 and 7-13, four 4DoF vertices at 4 rows each, pad rows identity / zero),
 * rhs, x, the solver's failure flag, and plan = [storage mode, stored blocks, blocks in LDS, levels, columns per level
 * ...] (plan_cap >= 4 + levels). */
omv_status omv_essgraph_debug_solve(omv_essgraph *h, double lambda, double *S, double *rhs, double *x, int32_t *fail,
                                    int32_t *plan, int plan_cap);
/* Blocks of the system of the current problem (for sizing debug_solve's arrays); 0 without a problem. */
omv_status omv_essgraph_blocks(omv_essgraph *h, int *n_blocks, int *n_levels);
/* The epilogue of the three functions from the device state.  poses [n_vertices][7] (optional): the Sophus::SE3f
 * handed to SetPose as unit quaternion (x y z w) and translation -- LOOP: rotation cast to float, t.cast<float>() / s;
 * MERGE: t / s in double, then the cast; 4DOF: (Rcw, tcw) of camera 0.  points [n_points][3] (in/out, float): point p
 * becomes correctedSwr.map(Srw.map(P)) in double, cast to float, with r = point_ref[p], Srw = S_a[r] and correctedSwr
 * the inverse of vertex r's estimate; point_ref -1 leaves the point untouched.  OMV_ERR_ARG: a mode that is not the
 * handle's kind's, a reference outside -1 .. n_vertices - 1. */
omv_status omv_essgraph_recover(omv_essgraph *h, int mode, float *poses, int n_points, float *points,
                                const int32_t *point_ref);
/* The pose graph is single-rank: always OMV_ERR_ARG. */
omv_status omv_essgraph_set_comm(omv_essgraph *h, int rank, int world, omv_allreduce_fn allreduce, void *ctx);
/* Device time of the last optimize() in milliseconds (events around its launches). */
omv_status omv_essgraph_last_ms(omv_essgraph *h, double *ms);

#ifdef __cplusplus
}
#endif
#endif /* OMV_H */
