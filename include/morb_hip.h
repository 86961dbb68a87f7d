/* morb_hip.h — C ABI of libmorb_hip.so: the MI355X (gfx950) implementation of MORB_SLAM's per-frame front end.
 *
 * The reference has no FFI layer: its boundary for this path is three C++ class surfaces called in-process
 * (SURVEY.md §8b).  Each entry point below names the reference interface it replaces (paths relative to the
 * reference root).  Plain pointers, sizes and PODs only; every function returns an int status
 * (MORB_OK = 0, negative = error) unless documented otherwise; no exceptions cross this boundary.
 * Pointers named d_* are DEVICE pointers (HIP), everything else is host memory.  `stream` is a hipStream_t
 * passed as void* (NULL = the handle's own stream).
 */
#ifndef MORB_HIP_H
#define MORB_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MORB_OK 0
#define MORB_ERR_INVALID (-1)   /* bad argument */
#define MORB_ERR_HIP (-2)       /* HIP runtime error; see morb_last_error() */
#define MORB_ERR_CAPACITY (-3)  /* caller buffer too small */
#define MORB_ERR_UNSUPPORTED (-4)
#define MORB_ERR_EMPTY (-5)     /* empty image: ORBextractor::operator() returns -1 (src/ORBextractor.cc:1011) */

/* cv::KeyPoint as the reference stores it (28 bytes): pt.x, pt.y, size, angle, response, octave, class_id */
typedef struct morb_keypoint {
  float x, y, size, angle, response;
  int32_t octave, class_id;
} morb_keypoint;

const char* morb_last_error(void);
int morb_device_count(void);

/* ------------------------------------------------------------------------------------------------------
 * ORBextractor  (include/ORBextractor.h:44-105, src/ORBextractor.cc)
 * ---------------------------------------------------------------------------------------------------- */
typedef struct morb_extractor morb_extractor;

/* ORBextractor::ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)  ORBextractor.h:49-50,
 * ORBextractor.cc:406-464.  `device` = HIP device ordinal. */
int morb_extractor_create(morb_extractor** out, int nfeatures, float scaleFactor, int nlevels, int iniThFAST,
                          int minThFAST, int device);
void morb_extractor_destroy(morb_extractor*);

/* GetLevels / GetScaleFactor / GetScaleFactors / GetInverseScaleFactors / GetScaleSigmaSquares /
 * GetInverseScaleSigmaSquares  (ORBextractor.h:59-74); arrays hold nlevels entries; any pointer may be NULL. */
int morb_extractor_levels(const morb_extractor*);
float morb_extractor_scale_factor(const morb_extractor*);
int morb_extractor_tables(const morb_extractor*, float* scaleFactors, float* invScaleFactors, float* sigma2,
                          float* invSigma2, int* featuresPerLevel);

/* Upper bound of keypoints one image can yield (size the kps/desc buffers with it). */
int morb_extractor_max_keypoints(const morb_extractor*);

/* int ORBextractor::operator()(image, mask (ignored), keypoints, descriptors, vLappingArea)
 * ORBextractor.h:55-57, ORBextractor.cc:1006-1086.  Host image in (CV_8UC1, `stride` bytes per row), host
 * keypoints (28 B each) and descriptors (32 B each) out, *n = number of keypoints.
 * Returns monoIndex (>= 0) exactly as the reference does, MORB_ERR_EMPTY for an empty image (reference: -1),
 * or another negative status.
 * `image` may be a cv::Mat with a step or a ROI of a larger frame: stride >= width, and only the `width` bytes of each row are read —
 * nothing between two rows, nothing beyond (height - 1) * stride + width.  Limits (MORB_ERR_UNSUPPORTED): stride < 2^24 and
 * stride * height < 2^32. */
int morb_extract(morb_extractor*, const uint8_t* image, int width, int height, int stride, int lap0, int lap1,
                 morb_keypoint* kps, uint8_t* desc, int cap, int* n);

/* Batched, device-resident form of operator(): nimg images of identical size, image i at
 * d_images + i*image_pitch.  lap = host array [nimg][2] of lapping areas, or NULL for {0,0} (the rectified
 * stereo call, Frame.cc:194-197).  Outputs are device arrays: d_kps [nimg][cap], d_desc [nimg][cap][32],
 * d_count [nimg], d_mono [nimg] (monoIndex); cap >= morb_extractor_max_keypoints() (else MORB_ERR_CAPACITY: the lapping-area
 * keypoints fill every image's range from the back).  Asynchronous on `stream`.
 * Rows lie `stride` bytes apart (stride >= width, any alignment of d_images), image_pitch >= stride * height; only the `width` bytes
 * of each row are read, and the images are never written.  Limits (MORB_ERR_UNSUPPORTED): stride < 2^24 and stride * height < 2^32,
 * what the 32-bit row offsets of the level-0 kernel carry. */
int morb_extract_batch(morb_extractor*, const uint8_t* d_images, int nimg, int width, int height, int stride,
                       size_t image_pitch, const int* lap, morb_keypoint* d_kps, uint8_t* d_desc, int cap,
                       int* d_count, int* d_mono, void* stream);

/* std::vector<cv::Mat> mvImagePyramid (public member, ORBextractor.h:76; read by
 * Frame::ComputeStereoMatches, Frame.cc:895,974,987).  Level `lvl` of image `img` of the last batch:
 * *d_ptr points at the interior origin (the cv::Mat ROI), *stride is the row pitch.  Of the reference's 19-px
 * BORDER_REFLECT_101 pad only the innermost 3 pixels — the ones the 7 x 7 blur reads — surround the interior in the
 * allocation; the other 16 are read by nothing and are not stored. */
int morb_extractor_pyramid_level(const morb_extractor*, int img, int lvl, const uint8_t** d_ptr, int* width,
                                 int* height, int* stride);
/* Same, copied to host with the reference's full pad: out is (height+38) x (width+38) contiguous.  The stored
 * (height+6) x (width+6) block is copied into the middle as it is; the outer 16-px ring is reconstructed on the host
 * by BORDER_REFLECT_101 of the interior. */
int morb_extractor_pyramid_level_host(const morb_extractor*, int img, int lvl, uint8_t* out_padded);
/* Debug/parity taps on the last batch (host copies): blurred level (height x width contiguous), FAST
 * candidates of a level in vToDistributeKeys order, keypoints of a level after DistributeOctTree. */
int morb_extractor_blurred_level_host(const morb_extractor*, int img, int lvl, uint8_t* out);
int morb_extractor_level_candidates_host(const morb_extractor*, int img, int lvl, morb_keypoint* out, int cap,
                                         int* n);
int morb_extractor_level_keypoints_host(const morb_extractor*, int img, int lvl, morb_keypoint* out, int cap,
                                        int* n);

/* Per-stage device time: with profiling enabled every morb_extract_batch records HIP events on its stream at
 * the stage boundaries (no host synchronisation in the call).  morb_extractor_stage_ms waits for the recorded
 * calls (at most the last 64), writes the per-call AVERAGE in ms for stages 0..6 = pyramid, blur, fast,
 * distribute, layout, describe, total, resets the window and returns the number of calls averaged.
 * Mirrors the reference's REGISTER_TIMES spans (src/Frame.cc:190-206). */
int morb_extractor_set_profiling(morb_extractor*, int enable);
int morb_extractor_stage_ms(morb_extractor*, float* ms7);
/* The event (hipEvent_t) the last morb_extract_batch recorded on its stream after the FAST stage — where the memory-bound half of the
 * extraction (pyramid, FAST's window loads) ends and the quadtree's mostly idle chip begins.  A caller that pipelines frames can make
 * another stream wait for it (hipStreamWaitEvent) so that other work — the previous frame's matchers — lands underneath the quadtree
 * instead of beside the next pyramid.  Owned by the handle; valid until the handle is destroyed. */
int morb_extractor_event_after_fast(morb_extractor*, void** event);
/* Likewise the event recorded behind the last pyramid launch (ComputePyramid, src/ORBextractor.cc:1088-1112), i.e. where the FAST stage starts:
 * k_fastw is bound by vector-instruction issue and leaves the memory pipe idle, so a pipelining caller may prefer to put the previous frame's
 * matchers (BoW descent, SAD rows: memory-pipe work) underneath IT rather than beside the pyramid, which needs the same pipe.
 * The event is recorded by the extractions queued AFTER the first call of this function on the handle (call it once before the first batch):
 * callers that never ask do not pay for an event between the pyramid and FAST. */
int morb_extractor_event_after_pyramid(morb_extractor*, void** event);
/* Failure flags raised on the device by the extractions since the last query (cleared by the call).  To be read AFTER the stream of a
 * morb_extract_batch call has been synchronised; morb_extract checks it itself.  Bit 0: a pyramid level held more than 65535 FAST
 * candidates (noise-like images; the quadtree counts children in 16 bits) -> returns MORB_ERR_UNSUPPORTED, that call's keypoints are not valid. */
int morb_extractor_status(morb_extractor*, int* flags);
/* hipStreamWaitEvent(stream, event) through the HIP runtime THIS library is linked against: a host language that holds raw stream /
 * event handles (ctypes, cgo) must not open a second copy of libamdhip64 to make `stream` wait for the event above. */
int morb_stream_wait_event(void* stream, void* event);

/* ------------------------------------------------------------------------------------------------------
 * Matchers: ORBmatcher (include/ORBmatcher.h:36-129, src/ORBmatcher.cc) and the per-frame stereo matchers
 * of Frame.cc.  The reference walks Frame/KeyFrame/MapPoint objects; the ABI takes the fields each function
 * reads, flattened: features of image i live at [i*cap, i*cap + count[i]) of the keypoint / descriptor arrays
 * (the layout morb_extract_batch writes).  All array arguments are DEVICE pointers; calls are asynchronous
 * on `stream` (NULL = the matcher's own stream).
 * ---------------------------------------------------------------------------------------------------- */
typedef struct morb_matcher morb_matcher;
int morb_matcher_create(morb_matcher** out, int device);
void morb_matcher_destroy(morb_matcher*);
/* Wait for the work queued on the matcher's OWN stream (calls made with stream = NULL) — not for the device: another handle's work
 * (a LocalBundleAdjustment trial on the mapping thread's optimizer, System.cc:209) keeps running. */
int morb_matcher_sync(morb_matcher*);
/* The matcher's own stream (hipStream_t): a host adapter queues its uploads / downloads there instead of on the null stream. */
void* morb_matcher_stream(const morb_matcher*);

/* Feature slabs — the unit one GPU ships to another (no counterpart in the single-process reference; north_star's frame sharding).
 * A frame matched against its predecessor (SearchByBoW / SearchByProjection(Cur, Last)) needs the predecessor's keypoints, descriptors and
 * BoW node ids; with frames dealt round-robin over GPUs they live on the previous GPU.  pack gathers S rows of the [nimg][cap] feature arrays
 * (row d_rows[f], or row f when d_rows is NULL — e.g. the left images 0, 2, 4, ...) into ONE contiguous buffer of morb_feature_slab_bytes(S, cap)
 * bytes: [S][cap] keypoints | [S][cap][32] descriptors | [S][cap] node ids (-1 when d_node is NULL) | [S] counts.  The caller moves that one
 * buffer (hipMemcpyPeerAsync over xGMI, or an RCCL send / recv) and unpack scatters it into rows d_rows[f] of the receiver's pool.  All
 * pointers are DEVICE pointers; asynchronous on `stream`.  INTEGRATION.md section 5 shows the sharding loop of a C++ Tracking.
 * PRECONDITIONS (not checked: the sizes live in device memory): the slab holds morb_feature_slab_bytes(S, cap) bytes; every d_rows[f]
 * (or f itself when d_rows is NULL) is a row of arrays allocated with the SAME cap as the packer's; the counts inside the slab are
 * <= cap (pack writes min(count, cap)).  A slab packed with another cap must not be unpacked: the row pitch is part of the format. */
size_t morb_feature_slab_bytes(int S, int cap);
int morb_feature_slab_pack(morb_matcher*, int S, int cap, const int* d_rows, const morb_keypoint* d_kps, const uint8_t* d_desc, const int* d_node,
                           const int* d_count, void* d_slab, void* stream);
int morb_feature_slab_unpack(morb_matcher*, int S, int cap, const void* d_slab, const int* d_rows, morb_keypoint* d_kps, uint8_t* d_desc, int* d_node,
                             int* d_count, void* stream);

/* static int ORBmatcher::DescriptorDistance(a, b)  ORBmatcher.h:43, ORBmatcher.cc:1880-1894; n pairs of 32-byte
 * descriptors -> n distances. */
int morb_hamming_pairs(morb_matcher*, const uint8_t* d_a, const uint8_t* d_b, int n, int* d_out, void* stream);

/* cv::BFMatcher(NORM_HAMMING).knnMatch(query, train, matches, 2) as Frame::ComputeStereoFishEyeMatches uses
 * it (Frame.cc:46, :1242).  Problem p: query rows [qOff[p], nq[p]) of d_query + p*qPitch*32, train rows
 * [tOff[p], nt[p]) likewise (qOff/tOff NULL = 0: monoLeft / monoRight in the reference).  Output for query row
 * r (relative to qOff): d_idx[(p*qPitch + r)*2 + {0,1}] = train index relative to tOff (-1 if absent),
 * d_dist likewise; ties: lower train index first. */
int morb_hamming_knn2_batch(morb_matcher*, int nprob, const uint8_t* d_query, const int* d_nq, int qPitch,
                            const int* d_qOff, const uint8_t* d_train, const int* d_nt, int tPitch, const int* d_tOff,
                            int* d_idx, int* d_dist, void* stream);

/* void Frame::ComputeStereoMatches()  Frame.cc:889-1047 for nframes rectified stereo frames whose images the
 * extractor has just processed in ONE batch with left = image 2f, right = image 2f+1 (it reads the
 * extractor's mvImagePyramid like the reference does, Frame.cc:895,974,987).  mbf, mb as Frame::mbf / mb.
 * Outputs mvuRight / mvDepth: d_uRight[f*cap + i], d_depth[f*cap + i] for left keypoint i (-1 = no match). */
int morb_stereo_match_batch(morb_matcher*, const morb_extractor*, int nframes, const morb_keypoint* d_kps,
                            const uint8_t* d_desc, const int* d_count, int cap, float mbf, float mb, float* d_uRight,
                            float* d_depth, void* stream);

/* void Frame::ComputeStereoFishEyeMatches()  Frame.cc:1222-1274 for nframes fisheye stereo frames (left = image 2f,
 * right = image 2f+1 of one extract batch): brute-force 2-NN over the lapping-area features (from index
 * d_mono[image] = the monoIndex ORBextractor::operator() returned), ratio 0.7, KannalaBrandt8::TriangulateMatches.
 * camL8 / camR8 (HOST) = fx fy cx cy k0..k3; Rlr9 / tlr3 (HOST) = Frame::mRlr / mtlr; levelSigma2 = mvLevelSigma2.
 * Outputs [nframes][cap]: mvLeftToRightMatch, mvRightToLeftMatch, mvDepth, mvStereo3Dpoints ([..][3]); d_nMatches[f]. */
int morb_stereo_fisheye_match_batch(morb_matcher*, int nframes, const morb_keypoint* d_kps, const uint8_t* d_desc,
                                    const int* d_count, const int* d_mono, int cap, const float* camL8, const float* camR8,
                                    const float* Rlr9, const float* tlr3, const float* levelSigma2, int nlevels,
                                    int* d_leftToRight, int* d_rightToLeft, float* d_depth, float* d_p3D, int* d_nMatches,
                                    void* stream);

/* DBoW2 TemplatedVocabulary::transform(feature, word_id, weight, nid, levelsup)
 * (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1218-1259) for every feature of nimg images: the vocabulary is
 * a k-ary tree in arrays (node 0 = root; children of n = firstChild[n] .. firstChild[n]+k-1; firstChild < 0 =
 * leaf; one 32-byte descriptor per node).  d_wordId = leaf node reached, d_nodeId = ancestor at level
 * L - levelsup: the FeatureVector key that SearchByBoW / SearchForTriangulation bucket on (Frame::ComputeBoW,
 * Frame.cc:822-827, levelsup = 4). */
int morb_bow_transform_batch(morb_matcher*, int nimg, const uint8_t* d_desc, const int* d_count, int cap,
                             const uint8_t* d_nodeDesc, const int* d_firstChild, int k, int L, int levelsup,
                             int* d_wordId, int* d_nodeId, void* stream);

/* The same descent on a trained vocabulary whose nodes may have fewer than k children (ORBvoc.txt: 1 082 073 nodes, not the
 * 1 111 111 of a complete 10-ary tree): children of node n are [d_firstChild[n], d_firstChild[n] + d_childCount[n]). */
int morb_bow_transform_tree_batch(morb_matcher* m, int nimg, const uint8_t* d_desc, const int* d_count, int cap,
                                  const uint8_t* d_nodeDesc, const int* d_firstChild, const int* d_childCount, int L, int levelsup,
                                  int* d_wordId, int* d_nodeId, void* stream);

/* DBoW2 text vocabulary (TemplatedVocabulary::loadFromTextFile, Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1338-1420;
 * SURVEY 8f N3): header "k L scoring weighting", then one node per line "parent isLeaf d0 .. d31 weight"; node ids in file
 * order from 1 (0 = root), word ids = order of the leaves.  Host-side loader; morb_vocabulary_arrays copies the flattened
 * tree (caller-allocated arrays of nNodes entries; any may be NULL) for upload to the device.  wordId[leaf node] maps the
 * transform's leaf node id to DBoW2's WordId. */
typedef struct morb_vocabulary morb_vocabulary;
int morb_vocabulary_load_text(const char* path, morb_vocabulary** out);
void morb_vocabulary_destroy(morb_vocabulary* v);
int morb_vocabulary_info(const morb_vocabulary* v, int* k, int* L, int* nNodes, int* nWords);
int morb_vocabulary_arrays(const morb_vocabulary* v, uint8_t* nodeDesc, int* firstChild, int* childCount, int* wordId, float* weight);
/* the node weights as DBoW2 holds them (WordValue = double) and the header's scoring / weighting types (BowVector.h:39-56:
 * weighting 0 TF_IDF, 1 TF, 2 IDF, 3 BINARY; scoring 0 L1_NORM .. 5 DOT_PRODUCT); any pointer may be NULL */
int morb_vocabulary_weights(const morb_vocabulary* v, double* weight, int* scoring, int* weighting);

/* The BowVector half of TemplatedVocabulary::transform(features, BowVector&, FeatureVector&, levelsup)
 * (TemplatedVocabulary.h:1127-1190, BowVector.cpp:34-84), for nimg images: d_leaf = the leaf NODE ids of the descent
 * (morb_bow_transform*'s d_wordId output), d_nodeWordId = node -> WordId (NULL: the node id itself), d_nodeWeight = node weights
 * (double).  Words with weight 0 are "stopped".  Outputs: the map's entries in ascending word order, d_bowWord / d_bowValue
 * [nimg][cap] and d_bowCount[nimg]. */
int morb_bow_vector_batch(morb_matcher*, int nimg, const int* d_leaf, const int* d_count, int cap, const int* d_nodeWordId,
                          const double* d_nodeWeight, int weighting, int scoring, int* d_bowWord, double* d_bowValue, int* d_bowCount,
                          void* stream);

/* void KeyFrameDatabase::DetectNBestCandidates(KeyFrame* pKF, vector<KeyFrame*>& vpLoopCand, vector<KeyFrame*>& vpMergeCand,
 * int nNumCandidates) (src/KeyFrameDatabase.cc:579-705; the call of LoopClosing.cc:484) for nq queries at once, with DBoW2's L1
 * score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68).  Only the L1 score is built, so there is no scoring argument: it is
 * ORBvoc.txt's and the only one the reference runs.  No inverted file is kept (add / erase / clear / clearMap, :37-93, become d_dbRank).
 *   pool      d_bowWord / d_bowValue [nimg][cap], d_bowCount [nimg]: exactly what morb_bow_vector_batch writes.
 *   d_qImg    [nq] pool row of each query (pKF->mBowVec is a pool row too); the query's map is d_mapId[d_qImg[q]].
 *   d_dbRank  [nimg] the keyframe's position in `add` order (unique among the rows that have one), negative = not in the database.
 *   d_connStart [nq + 1], d_conn: CSR of pKF->GetConnectedKeyFrames() per query, as pool rows.
 *   d_covis   [nimg][ncovis] GetBestCovisibilityKeyFrames(10) of each row, in its order, as pool rows, padded with -1.
 *   d_mapId   [nimg] the map of each row; d_flags [nimg]: bit 0 = isBad(), bit 1 = GetMap()->IsBad().
 *   d_prevScore [nimg] mPlaceRecognitionScore on entry, NULL = zeros; it must not be d_score.  EVERY query of the batch sees this
 *             entry state: a batch of one equals the reference call, a batch of n equals n independent calls on that state.
 * A keyframe is "stamped" by a query when it is in the database, shares a word with it and is not connected to it.  The entry takes
 * as given that a query id (pKF->mnId) never equals a stamp an earlier query left, nor the initial 0: ids are unique per query and
 * nonzero wherever the reference calls this.
 * Outputs: d_loopCand / d_mergeCand [nq][nNumCandidates] pool rows padded with -1, d_nLoop / d_nMerge [nq]; d_words [nq][nimg] =
 * mnPlaceRecognitionWords of a stamped keyframe, -1 otherwise; d_score [nq][nimg] = mPlaceRecognitionScore after the query (a
 * stamped keyframe that was not scored keeps d_prevScore's).  d_words and d_score may be NULL.  The candidate rows can be passed on
 * the device as d_kf2Img of morb_search_by_bow_kfkf_batch.  MORB_ERR_INVALID for a negative size, cap < 1, ncovis < 0 or
 * nNumCandidates < 1; nq == 0 or nimg == 0 is MORB_OK with nothing written. */
int morb_detect_n_best_candidates_batch(morb_matcher*, int nq, const int* d_qImg, int nimg, int cap, const int* d_bowWord,
                                        const double* d_bowValue, const int* d_bowCount, const int* d_dbRank, const int* d_connStart,
                                        const int* d_conn, const int* d_covis, int ncovis, const int* d_mapId, const uint8_t* d_flags,
                                        const float* d_prevScore, int nNumCandidates, int* d_loopCand, int* d_nLoop, int* d_mergeCand,
                                        int* d_nMerge, int* d_words, float* d_score, void* stream);

/* vector<KeyFrame*> KeyFrameDatabase::DetectRelocalizationCandidates(Frame* F, Map* pMap) (src/KeyFrameDatabase.cc:707-814; the call
 * of Tracking.cc:3369) for nq queries: as above with no connected set, d_qMap [nq] = pMap (a frame has no identity as a keyframe of
 * the pool), no sort, the entries with accScore > 0.75f * bestAccScore whose best keyframe lies in d_qMap[q], first occurrences, in
 * accumulation order.  d_cand [nq][nimg] pool rows padded with -1 (usable as d_kfImg of morb_search_by_bow_batch), d_nCand [nq];
 * d_words / d_score = mnRelocWords / mRelocScore (the reference's constructor leaves mRelocScore uninitialised: 0 here).  L1 only.
 * The same assumption on the query id (F->mnId against mnRelocQuery) and the same error codes. */
int morb_detect_relocalization_candidates_batch(morb_matcher*, int nq, const int* d_qImg, const int* d_qMap, int nimg, int cap,
                                                const int* d_bowWord, const double* d_bowValue, const int* d_bowCount,
                                                const int* d_dbRank, const int* d_covis, int ncovis, const int* d_mapId,
                                                const float* d_prevScore, int* d_cand, int* d_nCand, int* d_words, float* d_score,
                                                void* stream);

/* int ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches)
 * ORBmatcher.h:68, ORBmatcher.cc:218-395 (non-fisheye branch) for npairs (keyframe, frame) pairs drawn from a
 * pool of nimg images: pair p matches image d_kfImg[p] (as pKF) against image d_fImg[p] (as F).
 * d_node[i*cap + j] = FeatureVector node id of feature j (negative = not in the FeatureVector);
 * d_hasMP[i*cap + j] != 0 <=> vpMapPointsKF[j] is non-NULL and not bad.  nnratio / checkOri = the ORBmatcher
 * constructor arguments.  d_matchF[p*cap + j] = keyframe feature matched to frame feature j (-1 = none; the
 * adapter maps it to vpMapPointsKF[...]); d_nmatches[p] = the return value. */
int morb_search_by_bow_batch(morb_matcher*, int npairs, const int* d_kfImg, const int* d_fImg, int nimg,
                             const morb_keypoint* d_kps, const uint8_t* d_desc, const int* d_node, const int* d_count,
                             const uint8_t* d_hasMP, int cap, float nnratio, int checkOri, int* d_matchF,
                             int* d_nmatches, void* stream);

/* MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:367-435) for nMP map points at once: the observed
 * descriptors of point m (the rows the reference pushes into vDescriptors, in observation order) are rows
 * [d_start[m], d_start[m + 1]) of d_desc.  d_bestIdx[m] = index (within the point's rows) of the descriptor with the least
 * median Hamming distance to the others (first minimum), -1 for a point without descriptors; the caller clones that row
 * into mDescriptor.  At most 65535 descriptors per point. */
int morb_distinctive_descriptors_batch(morb_matcher* m, int nMP, const int* d_start, const uint8_t* d_desc, int* d_bestIdx,
                                       void* stream);

/* ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12) (ORBmatcher.cc:702-819; loop
 * closing / merging): both sides are keyframes of the pool; hasMP[img][i] != 0 <=> GetMapPointMatches()[i] && !isBad();
 * d_nValid[img] = mvKeysUn.size() (features at or beyond it are skipped on fisheye keyframes, :734 / :751; NULL = all).
 * match12[p][idx1] = index of the matched pKF2 feature or -1 (vpMatches12[idx1] = vpMapPoints2[match12]). */
int morb_search_by_bow_kfkf_batch(morb_matcher* m, int npairs, const int* d_kf1Img, const int* d_kf2Img, const int* d_nValid, int nimg,
                                  const morb_keypoint* d_kps, const uint8_t* d_desc, const int* d_node, const int* d_count,
                                  const uint8_t* d_hasMP, int cap, float nnratio, int checkOri, int* d_match12, int* d_nmatches,
                                  void* stream);

/* The same with a fisheye frame F (F.Nleft != -1, ORBmatcher.cc:262-299 and :333-365): image fImg[p] holds the
 * Nleft = d_nLeft[p] left features followed by the right ones; left and right candidates of a node are ranked
 * separately, the right winner is taken whenever the LEFT best distance passes TH_LOW (the reference's nesting and
 * its `|| true`).  d_nLeft[p] = -1 marks a pinhole frame. */
int morb_search_by_bow_fisheye_batch(morb_matcher* m, int npairs, const int* d_kfImg, const int* d_fImg, const int* d_nLeft,
                                     int nimg, const morb_keypoint* d_kps, const uint8_t* d_desc, const int* d_node,
                                     const int* d_count, const uint8_t* d_hasMP, int cap, float nnratio, int checkOri,
                                     int* d_matchF, int* d_nmatches, void* stream);

/* The Frame members the projection-guided searches read, as one POD (all frames of a batch share one camera):
 * mnMinX/Y, mnMaxX/Y, mfGridElementWidthInv/HeightInv, fx, fy, cx, cy, mbf, mb, mfLogScaleFactor, mnScaleLevels,
 * mvScaleFactors, mvLevelSigma2 (include/Frame.h). */
typedef struct morb_frame_params {
  float minX, minY, maxX, maxY, gridInvW, gridInvH;
  float fx, fy, cx, cy, mbf, mb, logScaleFactor;
  int32_t nlevels;
  float scaleFactors[16];
  float levelSigma2[16];
} morb_frame_params;

/* bool Frame::isInFrustum(MapPoint*, viewingCosLimit)  Frame.h / Frame.cc:611-678 (+ MapPoint::PredictScale,
 * MapPoint.cc:536-566) for d_nMP[f] map points of each of nframes frames (arrays [nframes][mpCap]).  Inputs:
 * d_Rcw [f][9] row-major, d_tcw [f][3], d_Ow [f][3] (Frame::mRcw, mtcw, mOw), world position, normal,
 * mfMaxDistance, mfMinDistance per point.  Outputs = the MapPoint tracking fields the function fills:
 * mbTrackInView, mTrackProjX, mTrackProjY, mTrackProjXR, mTrackDepth, mnTrackScaleLevel, mTrackViewCos. */
int morb_is_in_frustum_batch(morb_matcher*, const morb_frame_params*, int nframes, const float* d_Rcw, const float* d_tcw,
                             const float* d_Ow, int mpCap, const int* d_nMP, const float* d_Pw, const float* d_normal,
                             const float* d_maxDist, const float* d_minDist, float viewingCosLimit, uint8_t* d_inView,
                             float* d_projX, float* d_projY, float* d_projXR, float* d_depth, int* d_level,
                             float* d_viewCos, void* stream);

/* int ORBmatcher::SearchByProjection(Frame& F, const vector<MapPoint*>& vpMapPoints, th, bFarPoints, thFarPoints)
 * ORBmatcher.h:49-51, ORBmatcher.cc:42-209.  Frame f uses the features of image d_fImg[f]; d_uRight / d_blocked
 * are [nframes][cap] (mvuRight or NULL; blocked != 0 <=> mvpMapPoints[i] && Observations() > 0).  Map points
 * [nframes][mpCap] carry the fields isInFrustum wrote plus isBad, the representative descriptor and
 * hasObs (Observations() > 0).  d_matchF [nframes][cap] in/out: index of the map point assigned to feature i
 * (caller initialises to -1 or keeps earlier assignments); d_nmatches[f] = return value. */
int morb_search_by_projection_mps_batch(morb_matcher*, const morb_frame_params*, int nframes, const int* d_fImg, int cap,
                                        const int* d_count, const morb_keypoint* d_kps, const uint8_t* d_desc,
                                        const float* d_uRight, const uint8_t* d_blocked, int mpCap, const int* d_nMP,
                                        const uint8_t* d_inView, const uint8_t* d_isBad, const float* d_depth,
                                        const float* d_projX, const float* d_projY, const float* d_projXR, const int* d_level,
                                        const float* d_viewCos, const uint8_t* d_mpDesc, const uint8_t* d_mpHasObs, float th,
                                        int bFarPoints, float thFarPoints, float nnratio, int* d_matchF, int* d_nmatches,
                                        void* stream);

/* Fisheye (KannalaBrandt8) rig, Frame::isInFrustum with Nleft != -1 (Frame.cc:665-677) = Frame::isInFrustumChecks
 * (Frame.cc:1276-1346) once per camera.  One call = one camera: the caller passes mR, mt, twc exactly as :1283-1293
 * builds them (left: mRcw, mtcw, mOw; right: Rrl * mRcw, Rrl * mtcw + trl, mRwc * mTlr.translation() + mOw; row-major
 * 3x3 / 3 floats per frame) and that camera's parameters cam8 = fx fy cx cy k0 k1 k2 k3 (host pointer).  Outputs as
 * morb_is_in_frustum_batch minus mTrackProjXR: left call -> mbTrackInView, mTrackProjX/Y, mTrackDepth,
 * mnTrackScaleLevel, mTrackViewCos; right call -> mbTrackInViewR, mTrackProjXR/YR, mTrackDepthR, mnTrackScaleLevelR,
 * mTrackViewCosR.  Fields of a rejected point are -1 (the reference leaves them stale). */
int morb_is_in_frustum_kb8_batch(morb_matcher* m, const morb_frame_params* P, const float* cam8, int nframes, const float* d_R,
                                 const float* d_t, const float* d_twc, int mpCap, const int* d_nMP, const float* d_Pw,
                                 const float* d_normal, const float* d_maxDist, const float* d_minDist, float viewingCosLimit,
                                 uint8_t* d_inView, float* d_projX, float* d_projY, float* d_depth, int* d_level,
                                 float* d_viewCos, void* stream);

/* ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th, bFarPoints, thFarPoints) on a fisheye rig: the
 * F.Nleft != -1 branches of ORBmatcher.cc:42-209.  Image fImg[f] of the pool holds the Nleft left features followed
 * by the right ones (mvKeys | mvKeysRight, mDescriptors = vconcat, Frame.cc:211-214): count = N, d_nLeft[f] = Nleft.
 * d_l2r / d_r2l [nframes][cap] = mvLeftToRightMatch / mvRightToLeftMatch (local indices, -1 = none).  Left-camera
 * fields (*L) and right-camera fields (*R) come from the two morb_is_in_frustum_kb8_batch calls.  matchF[f][j] =
 * map point index claimed by feature j (left and right halves of the same table), -1 otherwise; nmatches as the
 * reference counts them (a stereo partner counts as a second match). */
int morb_search_by_projection_mps_fisheye_batch(morb_matcher* m, const morb_frame_params* P, int nframes, const int* d_fImg,
                                                int cap, const int* d_count, const int* d_nLeft, const morb_keypoint* d_kps,
                                                const uint8_t* d_desc, const int* d_l2r, const int* d_r2l,
                                                const uint8_t* d_blocked, int mpCap, const int* d_nMP,
                                                const uint8_t* d_inViewL, const uint8_t* d_inViewR, const uint8_t* d_isBad,
                                                const float* d_depthL, const float* d_projXL, const float* d_projYL,
                                                const int* d_levelL, const float* d_viewCosL, const float* d_projXR,
                                                const float* d_projYR, const int* d_levelR, const float* d_viewCosR,
                                                const uint8_t* d_mpDesc, const uint8_t* d_mpHasObs, float th, int bFarPoints,
                                                float thFarPoints, float nnratio, int* d_matchF, int* d_nmatches, void* stream);

/* ---- marshalling between the tracking-side searches and PoseOptimization for device-resident batches of frames ----
 * The host loops Tracking.cc runs between its calls (one frame, std::vector<MapPoint*>), restated for [nframes][cap]
 * tables in HBM so that SearchByProjection -> PoseOptimization -> isInFrustum -> SearchByProjection -> PoseOptimization
 * needs no host round trip (morb_slam_amd/tracking.py, bench.py's tracking chain).  The class adapters of include/morb/
 * do these steps on the host where the reference does.  A frame's map points are rows of a per-frame table
 * [nframes][mpCap]; "mvpMapPoints" is an index into it, -1 = NULL.
 *
 * void Frame::SetPose(Tcw) -> UpdatePoseMatrices()  src/Frame.cc:541-585.  d_pose7 [f][7] (unit quaternion xyzw +
 * translation, world -> camera) -> mRcw (row-major 9), mtcw, mOw = Tcw.inverse().translation(). */
int morb_frame_set_pose_batch(morb_matcher*, int nframes, const float* d_pose7, float* d_Rcw, float* d_tcw, float* d_Ow,
                              void* stream);
/* The unary edges Optimizer::PoseOptimization(Frame*) builds (src/Optimizer.cc:803-905): one per feature that holds a map
 * point; obs = (mvKeysUn[i].pt, mvuRight[i]) (mono edge when mvuRight < 0), invSigma2 = mvInvLevelSigma2[octave], Xw = the
 * map point's world position.  d_match == NULL: d_frameMP [f][cap] is read.  d_match != NULL: d_frameMP is WRITTEN from it,
 * through d_remap [f][remapCap] when given (SearchByProjection(Cur, Last) returns indices of last-frame features;
 * LastFrame.mvpMapPoints as indices is the remap).  Outputs are morb_pose_optimization_batch's inputs. */
int morb_pose_edges_batch(morb_matcher*, const morb_frame_params*, int nframes, const int* d_fImg, int cap, const int* d_count,
                          const morb_keypoint* d_kps, const float* d_uRight, const int* d_match, const int* d_remap, int remapCap,
                          int mpCap, const float* d_mpXw, int* d_frameMP, uint8_t* d_hasMP, float* d_obs, float* d_invSigma2,
                          float* d_Xw, void* stream);
/* Tracking::TrackWithMotionModel's outlier discard (src/Tracking.cc:2716-2740), SearchLocalPoints' first loop (:3117-3133)
 * and TrackLocalMap's inlier count (:2779-2806): features flagged by PoseOptimization lose their map point (d_outlier is
 * cleared), d_nmatches[f] = features that keep one, d_nmatchesMap[f] = those whose point has observations
 * (d_mpHasObs [f][mpCap], NULL = all), d_blocked [f][cap] (nullable) = the `mvpMapPoints[i] && Observations() > 0` flag
 * SearchByProjection(F, MapPoints) skips on, d_mpSeen [f][mpCap] (nullable) = mnLastFrameSeen == this frame (kept or just
 * lost): the points SearchLocalPoints must not project again. */
int morb_track_discard_outliers_batch(morb_matcher*, int nframes, const int* d_fImg, int cap, const int* d_count, int* d_frameMP,
                                      uint8_t* d_outlier, int mpCap, const uint8_t* d_mpHasObs, uint8_t* d_blocked,
                                      uint8_t* d_mpSeen, int* d_nmatches, int* d_nmatchesMap, void* stream);

/* void Tracking::UpdateLocalMap() (src/Tracking.cc:3184-3191) = UpdateLocalKeyFrames (:3220-3358) + UpdateLocalPoints (:3193-3218),
 * the step TrackLocalMap runs between the first PoseOptimization and SearchLocalPoints, for nq query frames at once on map tables
 * that stay on the device.  A batch of n equals n independent calls.  Every index is an int32 row, -1 = NULL; a row outside its
 * table is read as NULL, a count beyond its capacity as the capacity.  Integers only: two calls give identical bytes.
 * Map tables, shared by the queries.  Keyframes, nkf rows:
 *   d_kfMp [nkf][kfCap] mvpMapPoints as map-point rows, d_kfCount [nkf] = N; d_kfFlags [nkf]: bit 0 = isBad();
 *   d_kfOrder [nkf]   the keyframe's position in the iteration order of std::map<KeyFrame*, int> (:3222, :3271): a permutation of
 *                     0 .. nkf-1, taken as given; NULL = row order.  The reference orders by pointer value; here that order is data.
 *   d_covis [nkf][ncovis]  GetBestCovisibilityKeyFrames(10) in its order, padded with -1 (as morb_detect_n_best_candidates_batch's);
 *   d_childStart [nkf + 1] / d_child   CSR of GetChilds() in the set's iteration order (d_childStart NULL = no children);
 *   d_parent [nkf] GetParent(), d_prevKf [nkf] mPrevKF (either may be NULL = none).
 * Map points, nmp rows: d_mpObsStart [nmp + 1] / d_mpObsKf = CSR of the keys of GetObservations(), one entry per observing keyframe
 * (uniqueness is taken as given); d_mpFlags [nmp]: bit 0 = isBad().
 * Per query: d_frameMp [nq][cap] IN/OUT = mvpMapPoints of the voting frame as map-point rows (the caller passes the current or the
 * last frame's, the choice of :3223-3224); an entry whose point is bad is written to -1 (:3237 / :3257).  d_count [nq] = N;
 * d_lastKf [nq] = mCurrentFrame.mpLastKeyFrame (NULL = none); inertial != 0 <=> mSensor is one of the three IMU_* types (:3338).
 * What is reproduced, quirks included: every non-bad frame point votes for every keyframe of its observations, whatever the
 * keyframe's state; the voted, non-bad keyframes are listed in d_kfOrder order and pKFmax is the first of them with the strictly
 * greatest count (:3271-3285); the second loop (:3289-3335) runs over those entries only, stops when the list, additions included,
 * is larger than 80 at the top of an iteration, adds per entry the first non-bad unstamped covisible, the first non-bad unstamped
 * child and the unstamped parent, the parent without an isBad() test, and LEAVES THE LOOP after adding a parent (:3332); the
 * inertial tail (:3338-3352) runs below 80 entries, from d_lastKf along d_prevKf for at most 20 additions, ends at a stamped
 * keyframe and has no size test inside; the points (:3193-3218) are those of the listed keyframes in REVERSE list order, features
 * ascending, NULL, bad and already taken ones skipped.  The stamps a query starts from are clear.
 * Outputs: d_localKf [nq][kfOut], d_nLocalKf [nq] = mvpLocalKeyFrames; d_refKf [nq] = pKFmax, -1 = mpReferenceKF stays;
 * d_localMp [nq][mpCap], d_nLocalMp [nq] = mvpLocalMapPoints; d_frameLocal [nq][cap] (may be NULL) = the position of each feature's
 * point in d_localMp, -1 where it has none, where the point is not in the list (or at or beyond mpCap), and at or beyond d_count:
 * the per-frame table index the tracking entries above call "mvpMapPoints"; d_votes [nq][nkf] (may be NULL) = keyframeCounter, 0
 * where absent; d_overflow [nq]: bit 0 = the keyframe list is longer than kfOut, bit 1 = the point list is longer than mpCap; the
 * counts then hold the true lengths, the first kfOut / mpCap entries are correct and nothing is written beyond them.  Entries
 * beyond a count are not written.  Workspace on the handle: nq * (nkf + nmp) ints.
 * MORB_ERR_INVALID for a negative size or cap, kfCap, kfOut or mpCap < 1; MORB_ERR_CAPACITY for more than 65535 queries, or
 * nkf * kfCap or nq * (nkf + nmp) beyond 2^31 - 1.  nq == 0 is MORB_OK with nothing written; nkf == 0 or nmp == 0 is MORB_OK with
 * empty lists written. */
int morb_update_local_map_batch(morb_matcher*, int nq, int nkf, int kfCap, const int* d_kfMp, const int* d_kfCount,
                                const uint8_t* d_kfFlags, const int* d_kfOrder, const int* d_covis, int ncovis, const int* d_childStart,
                                const int* d_child, const int* d_parent, const int* d_prevKf, int nmp, const int* d_mpObsStart,
                                const int* d_mpObsKf, const uint8_t* d_mpFlags, int cap, int* d_frameMp, const int* d_count,
                                const int* d_lastKf, int inertial, int kfOut, int* d_localKf, int* d_nLocalKf, int* d_refKf, int mpCap,
                                int* d_localMp, int* d_nLocalMp, int* d_frameLocal, int* d_votes, int* d_overflow, void* stream);

/* The per-frame map-point tables Tracking::SearchLocalPoints (src/Tracking.cc:3117-3183) hands to isInFrustum and
 * SearchByProjection(F, mvpLocalMapPoints), filled from map-wide arrays through morb_update_local_map_batch's d_localMp [nq][mpCap]
 * / d_nLocalMp [nq].  Inputs [nmp]: world position (3 floats), normal (3), mfMaxDistance, mfMinDistance, the representative descriptor
 * (32 bytes), isBad(), Observations() > 0.  Outputs [nq][mpCap] in the layout morb_is_in_frustum_batch and
 * morb_search_by_projection_mps_batch take (d_nMP = d_nLocalMp; a count beyond mpCap is read as mpCap).  Rows at or beyond a query's
 * count are not written.  MORB_ERR_INVALID for a negative size or mpCap < 1; nq == 0 or nmp == 0 is MORB_OK with nothing written. */
int morb_gather_local_map_points_batch(morb_matcher*, int nq, int nmp, const float* d_mpPw, const float* d_mpNormal,
                                       const float* d_mpMaxDist, const float* d_mpMinDist, const uint8_t* d_mpDescriptor,
                                       const uint8_t* d_mpIsBad, const uint8_t* d_mpObserved, int mpCap, const int* d_localMp,
                                       const int* d_nLocalMp, float* d_Pw, float* d_normal, float* d_maxDist, float* d_minDist,
                                       uint8_t* d_mpDesc, uint8_t* d_isBad, uint8_t* d_mpHasObs, void* stream);

/* int ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono)
 * ORBmatcher.h:55-56, ORBmatcher.cc:1521-1733.  Frame pair f = (image d_curImg[f], image d_lastImg[f]); d_Tcw
 * [f][7] = CurrentFrame pose (quaternion xyzw + translation); per last-frame feature [nframes][cap]:
 * lastValid (map point present and not outlier), its world position, representative descriptor, hasObs.
 * d_bForward / d_bBackward [nframes]: the two flags of :1538-1539 (computed by the caller from the two poses).
 * d_matchCur [nframes][cap] in/out: index of the last-frame feature whose map point is assigned to current
 * feature i. */
int morb_search_by_projection_last_batch(morb_matcher*, const morb_frame_params*, int nframes, const int* d_curImg,
                                         const int* d_lastImg, int cap, const int* d_count, const morb_keypoint* d_kps,
                                         const uint8_t* d_desc, const float* d_curURight, const uint8_t* d_curBlocked,
                                         const float* d_Tcw, const uint8_t* d_lastValid, const float* d_lastXw,
                                         const uint8_t* d_lastMPdesc, const uint8_t* d_lastMPhasObs, float th,
                                         const uint8_t* d_bForward, const uint8_t* d_bBackward, int checkOri, int* d_matchCur,
                                         int* d_nmatches, void* stream);

/* The same with a fisheye current frame (CurrentFrame.Nleft != -1): left pass + right pass of ORBmatcher.cc:1521-1733.
 * Image curImg[f] holds the d_nLeftCur[f] left features followed by the right ones; cam8 = the LEFT camera's KB8
 * parameters (the reference projects both passes with mpCamera), Trl7 = GetRelativePoseTrl() as quaternion xyzw +
 * translation (host pointers).  Projections go through the device's atan2f / cosf / sinf (ulp-level differences from
 * the host libm can move a candidate that sits exactly on a window edge). */
int morb_search_by_projection_last_fisheye_batch(morb_matcher* m, const morb_frame_params* P, const float* cam8, const float* Trl7,
                                                 int nframes, const int* d_curImg, const int* d_lastImg, const int* d_nLeftCur,
                                                 int cap, const int* d_count, const morb_keypoint* d_kps, const uint8_t* d_desc,
                                                 const uint8_t* d_curBlocked, const float* d_Tcw, const uint8_t* d_lastValid,
                                                 const float* d_lastXw, const uint8_t* d_lastMPdesc,
                                                 const uint8_t* d_lastMPhasObs, float th, const uint8_t* d_bForward,
                                                 const uint8_t* d_bBackward, int checkOri, int* d_matchCur, int* d_nmatches,
                                                 void* stream);

/* int ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound, th, ORBdist)
 * ORBmatcher.h:60-62, ORBmatcher.cc:1735-1842 (relocalisation refinement).  Pair f = (current image d_curImg[f],
 * keyframe image d_kfImg[f]); d_Tcw [f][7], d_Ow [f][3] = Tcw.inverse().translation(); per keyframe feature
 * [nframes][cap]: kfValid (map point present, not bad, not in sAlreadyFound), world position, mfMaxDistance,
 * mfMinDistance, representative descriptor.  d_curHasMP [nframes][cap] != 0 <=> CurrentFrame.mvpMapPoints[i].
 * d_matchCur in/out as in the last-frame variant. */
int morb_search_by_projection_kf_batch(morb_matcher*, const morb_frame_params*, int nframes, const int* d_curImg,
                                       const int* d_kfImg, int cap, const int* d_count, const morb_keypoint* d_kps,
                                       const uint8_t* d_desc, const uint8_t* d_curHasMP, const float* d_Tcw, const float* d_Ow,
                                       const uint8_t* d_kfValid, const float* d_Xw, const float* d_maxDist,
                                       const float* d_minDist, const uint8_t* d_mpDesc, float th, int ORBdist, int checkOri,
                                       int* d_matchCur, int* d_nmatches, void* stream);

/* The same member when CurrentFrame is a KannalaBrandt8 rig frame (CurrentFrame.Nleft != -1).  The reference has no rig branch here: it
 * projects with CurrentFrame.mpCamera (cam8 = the LEFT camera's fx fy cx cy k0..k3, host pointer) and GetFeaturesInArea's bRight
 * defaults to false, so only the current frame's left features [0, d_nLeftCur[f]) are searched; rows hold left | right features.
 * Rotation check: the reference reads pKF->mvKeysUn[i] for every keyframe map point i, which is out of bounds for the keyframe's RIGHT
 * features (mvKeysUn holds the NLeft left keypoints); here feature i's own keypoint is used — mvKeysRight[i - NLeft] for a right
 * feature — i.e. row entry i of the keyframe image. */
int morb_search_by_projection_kf_rig_batch(morb_matcher*, const morb_frame_params*, const float* cam8, int nframes, const int* d_curImg,
                                           const int* d_kfImg, const int* d_nLeftCur, int cap, const int* d_count,
                                           const morb_keypoint* d_kps, const uint8_t* d_desc, const uint8_t* d_curHasMP, const float* d_Tcw,
                                           const float* d_Ow, const uint8_t* d_kfValid, const float* d_Xw, const float* d_maxDist,
                                           const float* d_minDist, const uint8_t* d_mpDesc, float th, int ORBdist, int checkOri,
                                           int* d_matchCur, int* d_nmatches, void* stream);


/* int ORBmatcher::SearchForInitialization(Frame& F1, Frame& F2, vbPrevMatched, vnMatches12, windowSize)
 * ORBmatcher.h:80-82, ORBmatcher.cc:603-700 (monocular initialisation).  Pair p = (image d_img1[p], image d_img2[p]);
 * d_prevMatched [npairs][cap][2] in/out (vbPrevMatched); d_matches12 [npairs][cap] = vnMatches12. */
int morb_search_for_initialization_batch(morb_matcher*, const morb_frame_params*, int npairs, const int* d_img1,
                                         const int* d_img2, int cap, const int* d_count, const morb_keypoint* d_kps,
                                         const uint8_t* d_desc, float* d_prevMatched, int windowSize, float nnratio,
                                         int checkOri, int* d_matches12, int* d_nmatches, void* stream);

/* int ORBmatcher::SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2, vMatchedPairs, bOnlyStereo, bCoarse)
 * ORBmatcher.h:84-87, ORBmatcher.cc:821-1042 (pinhole keyframes, no second camera) for npairs keyframe pairs of
 * a pool of nimg images (arrays [nimg][cap]; d_uRight may be NULL).  R12, t12 (HOST, [npairs][9], [npairs][3]) =
 * T1w * Tw2; ep (HOST [npairs][2]) = projection of KF1's centre into KF2 (:832-835).  d_match12 [npairs][cap] =
 * vMatches12 (feature of KF2 matched to feature i of KF1, -1 = none; the pair list is its non-negative entries in
 * ascending i), d_nmatches = return value. */
int morb_search_for_triangulation_batch(morb_matcher*, const morb_frame_params*, int npairs, const int* d_img1,
                                        const int* d_img2, int nimg, int cap, const int* d_count, const morb_keypoint* d_kps,
                                        const uint8_t* d_desc, const int* d_node, const uint8_t* d_hasMP, const float* d_uRight,
                                        const float* R12, const float* t12, const float* ep, int bOnlyStereo, int bCoarse,
                                        int checkOri, int* d_match12, int* d_nmatches, void* stream);

/* SearchForTriangulation between two keyframes of a KannalaBrandt8 rig (pKF->mpCamera2 != NULL, ORBmatcher.cc:845-852,
 * :884, :925, :934-975): each image holds its left features (d_nLeft1[p] / d_nLeft2[p] of them) followed by the right
 * ones; T4 = [npairs][4][12] host floats: Tll, Tlr, Trl, Trr (T1w * Tw2, T1w * Twr2, Tr1w * Tw2, Tr1w * Twr2), each
 * as rotation matrix (row-major) then translation.  bStereo is false on such rigs (bOnlyStereo rejects everything),
 * there is no epipole-distance gate, and the constraint is KannalaBrandt8::epipolarConstrain (TriangulateMatches >
 * 1e-4) with the cameras / relative pose of the two features' sides.  P->levelSigma2 = mvLevelSigma2. */
int morb_search_for_triangulation_fisheye_batch(morb_matcher* m, const morb_frame_params* P, int npairs, const int* d_img1,
                                                const int* d_img2, const int* d_nLeft1, const int* d_nLeft2, int nimg, int cap,
                                                const int* d_count, const morb_keypoint* d_kps, const uint8_t* d_desc,
                                                const int* d_node, const uint8_t* d_hasMP, const float* camL8, const float* camR8,
                                                const float* T4, int bOnlyStereo, int bCoarse, int checkOri, int* d_match12,
                                                int* d_nmatches, void* stream);

/* The body of LocalMapping::CreateNewMapPoints between SearchForTriangulation and Fuse (LocalMapping.cc:489-709) for npairs keyframe
 * pairs (current keyframe d_img1[p], neighbour d_img2[p]) of a pool of nimg pinhole images, mono or stereo (d_uRight / d_depth =
 * mvuRight / mvDepth, both NULL = monocular; d_kpsRaw = mvKeys for UnprojectStereo, NULL = d_kps, which is mvKeysUn).  d_match12
 * [npairs][cap] as morb_search_for_triangulation_batch wrote it; an entry at or beyond keyframe 2's count is no match.  Callers do not
 * submit the pairs the baseline gate rejects (:454-466, nmp_pair_gate of morb/new_map_points_math.h).
 * HOST arrays, as R12 / t12 of the search: poses [npairs][4][12] = Tcw1, Twc1, Tcw2, Twc2, each a 3 x 4 row-major [R | t] (GetPose() and
 * GetPoseInverse(); Ow = the translation of Twc); kf2First [npairs] != 0 <=> std::less<KeyFrame*>()(pKF2, mpCurrentKeyFrame), the order of
 * the new point's observation map, which decides the descriptor ComputeDistinctiveDescriptors keeps.  ratioFactor = 1.5f * mfScaleFactor.
 * Outputs per pair: d_status [npairs][cap] (NewMapPointStatus of morb/new_map_points_math.h, one code per `continue` of the reference),
 * d_stats [npairs][5] = created, totalStereoPts, countStereoAttempt, countStereoGoodProj, countStereo.
 * Outputs into the caller's tables [nrows][cap], pair p writing row d_row[p] (the current keyframe's feature-indexed point table, the
 * layout morb_fuse_batch takes with mpCap = cap) and only at accepted i: d_Xw [..][3], d_normal [..][3], d_maxDist, d_minDist
 * (UpdateNormalAndDepth), d_mpDesc [..][32] (ComputeDistinctiveDescriptors), d_obsImg2 / d_obsIdx2 (the second observation).
 * d_hasMP [nimg][cap] is updated in place by plain byte stores of 1 at [img1][i] and [img2][idx2] of accepted matches (AddMapPoint,
 * :700-701), so that the next neighbour's search skips those features: the reference's order is one launch per neighbour rank, rank k
 * of every current keyframe of a batch.  Pairs of one launch should not share an image; sharing one is harmless, the stores being
 * idempotent, but such a pair does not see the other's points.  A pair whose image or row index lies outside the tables writes -1 to
 * its stats and nothing else.  MORB_ERR_INVALID before any launch for a NULL array, a size below 1, nlevels outside [1, 16], only one of
 * d_uRight / d_depth, or mbFarPoints without a positive mThFarPoints; MORB_ERR_UNSUPPORTED for cap > 32768. */
int morb_create_new_map_points_batch(morb_matcher* m, const morb_frame_params* P, int npairs, const int* d_img1, const int* d_img2,
                                     int nimg, int cap, const int* d_count, const morb_keypoint* d_kps, const morb_keypoint* d_kpsRaw,
                                     const uint8_t* d_desc, const float* d_uRight, const float* d_depth, const int* d_match12,
                                     const float* poses, const uint8_t* kf2First, float ratioFactor, int mbInertial, int mbFarPoints,
                                     float mThFarPoints, int* d_status, int* d_stats, int nrows, const int* d_row, float* d_Xw,
                                     float* d_normal, float* d_maxDist, float* d_minDist, uint8_t* d_mpDesc, int* d_obsImg2,
                                     int* d_obsIdx2, uint8_t* d_hasMP, void* stream);

/* The same between two keyframes of a KannalaBrandt8 rig (:520-567), in the layout of morb_search_for_triangulation_fisheye_batch: left
 * features, then right.  Camera, pose and centre are those of the sides of idx1 and idx2; bStereo is false on a rig; mfMaxDistance is
 * still measured from the current keyframe's LEFT centre.  poses [npairs][8][12] = Tcw1, Twc1, Trw1, Twr1, Tcw2, Twc2, Trw2, Twr2
 * (GetPose(), its inverse, GetRightPose(), its inverse). */
int morb_create_new_map_points_fisheye_batch(morb_matcher* m, const morb_frame_params* P, int npairs, const int* d_img1,
                                             const int* d_img2, const int* d_nLeft1, const int* d_nLeft2, int nimg, int cap,
                                             const int* d_count, const morb_keypoint* d_kps, const uint8_t* d_desc, const float* camL8,
                                             const float* camR8, const int* d_match12, const float* poses, const uint8_t* kf2First,
                                             float ratioFactor, int mbInertial, int mbFarPoints, float mThFarPoints, int* d_status,
                                             int* d_stats, int nrows, const int* d_row, float* d_Xw, float* d_normal, float* d_maxDist,
                                             float* d_minDist, uint8_t* d_mpDesc, int* d_obsImg2, int* d_obsIdx2, uint8_t* d_hasMP,
                                             void* stream);

/* ---- M7: loop-closing / local-mapping searches ---------------------------------------------------------
 * Common inputs: problem f searches keyframe image d_kfImg[f] of the pool; map points are [nprob][mpCap] arrays;
 * d_valid[f][i] != 0 <=> the point passes the reference's state checks at the top of its loop (non-null, !isBad(),
 * !IsInKeyFrame(pKF) / !spAlreadyFound.count(pMP)); d_maxDist / d_minDist = mfMaxDistance / mfMinDistance (the 1.2 /
 * 0.8 factors of Get{Max,Min}DistanceInvariance are applied inside); poses are quaternion xyzw + translation.
 *
 * ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, th, bRight) (ORBmatcher.cc:1044-1213) and
 * Fuse(KeyFrame*, Sim3f& Scw, vpPoints, th, vpReplacePoint) (:1215-1321; sim3Form != 0: no reprojection gate, the caller
 * passes Tcw = SE3(Scw.rotationMatrix(), Scw.translation() / Scw.scale()) and Ow = Tcw.inverse().translation()).
 * Output: d_bestIdx[f][i] = feature chosen for map point i (bestDist <= TH_LOW) or -1, d_bestDist likewise (may be NULL).
 * The map-graph bookkeeping that follows a hit (Replace / AddObservation / AddMapPoint, :1196-1208, :1303-1310) depends on
 * live map state and stays with the caller, which replays the reference loop over these per-point results.
 * bRight on a fisheye rig: pass the right camera's pose / centre, cam8 = mpCamera2's KB8 parameters (host pointer, NULL =
 * the pinhole of P), d_jLo / d_jHi = [NLeft, N) per problem (NULL = all features) and d_uRight = NULL.  The Sim3 form on a rig keyframe (no rig
 * branch in the reference: pCamera = pKF->mpCamera, left features): cam8 = mpCamera's parameters, d_jLo / d_jHi = [0, NLeft). */
int morb_fuse_batch(morb_matcher* m, const morb_frame_params* P, int nprob, const int* d_kfImg, int cap, const int* d_count,
                    const morb_keypoint* d_kps, const uint8_t* d_desc, const float* d_uRight, const float* d_Tcw, const float* d_Ow,
                    const float* cam8, const int* d_jLo, const int* d_jHi, int mpCap, const int* d_nMP, const uint8_t* d_valid,
                    const float* d_Pw, const float* d_normal, const float* d_maxDist, const float* d_minDist,
                    const uint8_t* d_mpDesc, float th, int sim3Form, int* d_bestIdx, int* d_bestDist, void* stream);

/* ORBmatcher::SearchByProjection(KeyFrame*, Sim3f& Scw, vpPoints, vpMatched, th, ratioHamming) (:397-494) and its twin
 * with vpPointsKFs / vpMatchedKF (:496-601, manualProjection != 0: u = fx * (X * (1 / Z)) + cx instead of
 * mpCamera->project).  Tcw / Ow from Scw as above.  d_matched[f][idx] != 0 <=> vpMatched[idx] on entry.  Map points are
 * visited in order; a match blocks its feature.  d_matchF[f][idx] = index of the map point newly assigned to feature idx
 * or -1 (the caller writes vpMatched / vpMatchedKF from it); d_nmatches as returned by the reference. */
int morb_search_by_projection_sim3_batch(morb_matcher* m, const morb_frame_params* P, int nprob, const int* d_kfImg, int cap,
                                         const int* d_count, const morb_keypoint* d_kps, const uint8_t* d_desc, const float* d_Tcw,
                                         const float* d_Ow, int mpCap, const int* d_nMP, const uint8_t* d_valid, const float* d_Pw,
                                         const float* d_normal, const float* d_maxDist, const float* d_minDist,
                                         const uint8_t* d_mpDesc, const uint8_t* d_matched, int th, float ratioHamming,
                                         int manualProjection, int* d_matchF, int* d_nmatches, void* stream);

/* ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, S12, th) (:1323-1519).  Per pair: T1w / T2w = GetPose(); S12 and S21 =
 * S12.inverse() as 7 floats each (RxSO3 quaternion xyzw whose squared norm is the scale, then the translation).  d_valid1[p][i1]
 * != 0 <=> vpMapPoints1[i1] && !vbAlreadyMatched1[i1] && !isBad() (likewise 2); per-feature map-point arrays are [npairs][cap].
 * Outputs: d_vnMatch1 / d_vnMatch2 (the two one-way tables), d_match12[p][i1] = idx2 for mutually consistent pairs else -1,
 * d_nFound. */
int morb_search_by_sim3_batch(morb_matcher* m, const morb_frame_params* P, int npairs, const int* d_kf1Img, const int* d_kf2Img, int cap,
                              const int* d_count, const morb_keypoint* d_kps, const uint8_t* d_desc, const float* d_T1w,
                              const float* d_T2w, const float* d_S12, const float* d_S21, const uint8_t* d_valid1, const float* d_Pw1,
                              const float* d_maxDist1, const float* d_minDist1, const uint8_t* d_mpDesc1, const uint8_t* d_valid2,
                              const float* d_Pw2, const float* d_maxDist2, const float* d_minDist2, const uint8_t* d_mpDesc2,
                              float th, int* d_vnMatch1, int* d_vnMatch2, int* d_match12, int* d_nFound, void* stream);

/* The loop-closing searches on keyframes of a KannalaBrandt8 rig (KeyFrame::NLeft != -1; the feature row holds mvKeys | mvKeysRight).  The reference has no
 * rig branch in them: pKF->GetFeaturesInArea(u, v, r) defaults to bRight = false and mvKeysUn is the copy of mvKeys, so only the LEFT camera's features
 * [0, NLeft) are candidates (d_nLeft*[p] = NLeft), while every map point of the keyframe (left and right indices) is projected.
 * SearchByProjection(pKF, Scw, ...) (:397-494) projects with pKF->mpCamera->project (:433) = the left KB8 camera: cam8 (HOST, fx fy cx cy k0..k3); its twin
 * with vpPointsKFs (:496-601, manualProjection != 0) and SearchBySim3 (:1323-1519) keep the pinhole formula on pKF->fx, fy, cx, cy (:536-543, :1375-1379),
 * i.e. P's — cam8 is ignored there.  Everything else as in the two entry points above. */
int morb_search_by_projection_sim3_rig_batch(morb_matcher* m, const morb_frame_params* P, int nprob, const int* d_kfImg, int cap,
                                             const int* d_count, const morb_keypoint* d_kps, const uint8_t* d_desc, const float* d_Tcw,
                                             const float* d_Ow, int mpCap, const int* d_nMP, const uint8_t* d_valid, const float* d_Pw,
                                             const float* d_normal, const float* d_maxDist, const float* d_minDist,
                                             const uint8_t* d_mpDesc, const uint8_t* d_matched, int th, float ratioHamming,
                                             int manualProjection, const float* cam8, const int* d_nLeft, int* d_matchF, int* d_nmatches,
                                             void* stream);
int morb_search_by_sim3_rig_batch(morb_matcher* m, const morb_frame_params* P, int npairs, const int* d_kf1Img, const int* d_kf2Img, int cap,
                                  const int* d_count, const morb_keypoint* d_kps, const uint8_t* d_desc, const float* d_T1w,
                                  const float* d_T2w, const float* d_S12, const float* d_S21, const uint8_t* d_valid1, const float* d_Pw1,
                                  const float* d_maxDist1, const float* d_minDist1, const uint8_t* d_mpDesc1, const uint8_t* d_valid2,
                                  const float* d_Pw2, const float* d_maxDist2, const float* d_minDist2, const uint8_t* d_mpDesc2,
                                  float th, const int* d_nLeft1, const int* d_nLeft2, int* d_vnMatch1, int* d_vnMatch2, int* d_match12,
                                  int* d_nFound, void* stream);


/* ---- Frame-side helpers of the non-rectified / RGB-D input paths ----
 * void Frame::UndistortKeyPoints()  Frame.h, Frame.cc:829-857: cv::undistortPoints(mvKeys, K, mDistCoef, I, mK) for nimg images
 * (DEVICE pointers, image i at offset i*cap; d_count NULL = cap).  dist5 (HOST) = k1 k2 p1 p2 k3 (mDistCoef, k3 = 0 when it has
 * four entries); dist5[0] == 0 copies the records (:830-833).  Only pt.x / pt.y differ between d_kps and d_kpsUn. */
int morb_undistort_keypoints_batch(morb_matcher*, int nimg, int cap, const int* d_count, const morb_keypoint* d_kps, float fx,
                                   float fy, float cx, float cy, const float* dist5, morb_keypoint* d_kpsUn, void* stream);
/* void Frame::ComputeStereoFromRGBD(const cv::Mat& imDepth)  Frame.cc:1049-1067: d_depth = CV_32F depth images (already scaled
 * by mDepthMapFactor), row / image pitches in floats; outputs mvuRight / mvDepth ([nimg][cap], -1 where the depth is <= 0). */
int morb_stereo_from_rgbd_batch(morb_matcher*, int nimg, int cap, const int* d_count, const morb_keypoint* d_kps,
                                const morb_keypoint* d_kpsUn, const float* d_depth, int width, int height, size_t rowPitchFloats,
                                size_t imagePitchFloats, float bf, float* d_uRight, float* d_depthOut, void* stream);
/* void Frame::ComputeImageBounds(const cv::Mat& imLeft)  Frame.cc:859-887 (host): bounds4 = mnMinX, mnMaxX, mnMinY, mnMaxY. */
int morb_image_bounds(int width, int height, float fx, float fy, float cx, float cy, const float* dist5, float* bounds4);

/* ------------------------------------------------------------------------------------------------------
 * Optimizer  (include/Optimizer.h:46-139, src/Optimizer.cc; g2o Levenberg-Marquardt semantics)
 * Poses cross the boundary the way the reference hands them to g2o: unit quaternion (x, y, z, w) followed by
 * the translation, 7 floats (Sophus::SE3f::unit_quaternion() / translation(), Optimizer.cc:781-783, :1046-1048).
 * Pinhole mono (uRight < 0) and rectified-stereo (uRight >= 0) observations; PoseOptimization also for the
 * KannalaBrandt8 fisheye rig ("ToBody" edges), and so has LocalBundleAdjustment (morb_local_bundle_adjustment_fisheye).
 * ---------------------------------------------------------------------------------------------------- */
typedef struct morb_optimizer morb_optimizer;
int morb_optimizer_create(morb_optimizer** out, int device);
void morb_optimizer_destroy(morb_optimizer*);
/* Wait for the work queued on the optimizer's OWN stream (calls made with stream = NULL), not for the device. */
int morb_optimizer_sync(morb_optimizer*);
void* morb_optimizer_stream(const morb_optimizer*);   /* the optimizer's own stream (hipStream_t) */
/* PoseOptimization's deterministic mode.  on (the default since round 5): the sums over the edges (H, b, the robustified chi2) are taken in
 * edge order, one addition after the other, as g2o's sequential loop over its id-sorted active edges does (sparse_optimizer.cpp:482-487):
 * iterations AND trials are then g2o's, decision for decision (tests/test_optimizer_gpu.py).  The ordered sums run on the FP64 matrix core
 * (v_mfma_f64_4x4x4_4b_f64 adds its four products one after the other, each rounded: four edges per instruction) when the device passes the
 * self-test of morb_optimizer_create, on dependent v_add_f64 otherwise — the same bits either way.
 * off: per-thread partial sums and a tree — the reference's poses to ~1e-9, identical outlier flags, inlier counts and outer iterations; near
 * convergence rho = dChi2 / scale is ~0 and its sign follows the last bits of those sums, so the number of LM TRIALS can differ by one
 * (observed: 50 vs 49 in one of nine problems).  ~3 % faster per 256-frame batch (round 4: 1.7 x; the edge-order mode has closed the gap). */
int morb_optimizer_set_exact_order(morb_optimizer*, int on);
/* Which PoseOptimization path this handle runs (any out pointer may be NULL): *exact_order = the mode above; *mfma_chain = 1 when the edge-order sums
 * are carried by v_mfma_f64_4x4x4 (four edges per instruction), 0 when by dependent v_add_f64 — the order being reproduced is g2o's accumulation over
 * its active edges (Thirdparty/g2o/g2o/core/base_unary_edge.hpp:43-72 constructQuadraticForm, called edge by edge from
 * sparse_optimizer.cpp:482-487); *mfma_selftest = what the create-time self-test said on this device: 1 passed, 0 REJECTED the device (the vector chain
 * runs, same bits, slower), -1 not run (MORB_PO2_CHAIN=valu|mfma forced the choice) or could not run.  bench.py prints all three. */
int morb_optimizer_info(const morb_optimizer*, int* mfma_chain, int* exact_order, int* mfma_selftest);

/* static int Optimizer::PoseOptimization(Frame* pFrame)  Optimizer.h:86, Optimizer.cc:762-1051, for nframes
 * frames at once (DEVICE pointers, frame f at offset f*cap): d_count[f] = Frame::N (NULL = cap),
 * d_hasMP[i] != 0 <=> mvpMapPoints[i], d_obs[i] = (mvKeysUn[i].pt.x, .pt.y, mvuRight[i]),
 * d_invSigma2[i] = mvInvLevelSigma2[octave], d_Xw[i] = MapPoint world position; fx..bf = Frame::fx, fy, cx, cy,
 * mbf.  d_pose [nframes][7] in/out (Frame::GetPose / SetPose), d_outlier[i] = mvbOutlier[i],
 * d_nInliers[f] = the return value (0 when fewer than 3 correspondences; the pose is then left untouched).
 * d_stats (optional) [nframes][2] = outer LM iterations, LM trials. */
int morb_pose_optimization_batch(morb_optimizer*, int nframes, int cap, const int* d_count, const uint8_t* d_hasMP,
                                 const float* d_obs, const float* d_invSigma2, const float* d_Xw, float fx, float fy,
                                 float cx, float cy, float bf, float* d_pose, uint8_t* d_outlier, int* d_nInliers,
                                 int* d_stats, void* stream);

/* PoseOptimization for a fisheye stereo rig (pFrame->mpCamera2 != NULL: Optimizer.cc:880-946): features
 * [0, d_nLeft[f]) are left-camera observations (EdgeSE3ProjectXYZOnlyPose on the left KannalaBrandt8 camera), the rest
 * right-camera ones (EdgeSE3ProjectXYZOnlyPoseToBody with mTrl).  d_obs[i] = (x, y, unused).  camL8 / camR8 (HOST) =
 * fx fy cx cy k0 k1 k2 k3; Trl7 (HOST) = Frame::GetRelativePoseTrl() as quaternion xyzw + translation. */
int morb_pose_optimization_fisheye_batch(morb_optimizer*, int nframes, int cap, const int* d_count, const int* d_nLeft,
                                         const uint8_t* d_hasMP, const float* d_obs, const float* d_invSigma2,
                                         const float* d_Xw, const float* camL8, const float* camR8, const float* Trl7,
                                         float* d_pose, uint8_t* d_outlier, int* d_nInliers, int* d_stats, void* stream);

/* Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale, mAcumHessian, bAllPoints)  src/Optimizer.cc:2065-2322
 * (include/Optimizer.h:97-101), nprob problems, one workgroup each, asynchronous on `stream` (NULL = the handle's own).
 * Per KF1 feature i < d_count[p] (NULL = cap), arrays [nprob][cap]:
 *   d_entry  bit 0 vpMatches1[i] != NULL, bit 1 pMP1 = pKF1->GetMapPointMatches()[i] != NULL, bit 2 pMP1->isBad(), bit 3 pMP2->isBad();
 *   d_Xw1 / d_Xw2 [..][3] GetWorldPos() of pMP1 / pMP2; d_i2 = get<0>(pMP2->GetIndexInKeyFrame(pKF2));
 *   d_obs1 [..][2] = pKF1->mvKeysUn[i].pt, d_invSigma2_1 = pKF1->mvInvLevelSigma2[its octave];
 *   d_obs2 [..][2] = pKF2->mvKeysUn[i2].pt (unused when i2 < 0), d_invSigma2_2 = pKF2->mvInvLevelSigma2[octave of that keypoint]; when
 *   i2 < 0 the reference reads mvInvLevelSigma2[0]: its stand-in keypoint cv::KeyPoint(pt, pMP2->mnTrackScaleLevel) takes the level as
 *   the SIZE argument and keeps octave 0.
 * Per problem: d_T1w / d_T2w [12] = R row-major + t (float); d_cam1 / d_cam2 [9] = kind (0 Pinhole, 1 KannalaBrandt8) + the 8 parameters
 * of pKF1->mpCamera / pKF2->mpCamera; d_th2; d_fixScale; d_S12 [8] in / out = qx qy qz qw tx ty tz s (g2o::Sim3, doubles).
 * Outputs: d_keep[p][i] = vpMatches1[i] != NULL on return; d_nIn[p] = the return value; d_stats[p][8] = LM iterations and trials of
 * optimize(5), of the second optimize, 1 if the function reached its end (it then zeroes mAcumHessian and writes g2oS12; an early return
 * at nCorrespondences - nBad < 10 leaves both, but its nulled matches stay nulled), nCorrespondences, nBad, nIn.
 * Reproduced as the reference runs them:
 *   * an edge pair (EdgeSim3ProjectXYZ, EdgeInverseSim3ProjectXYZ) per match with both points good, skipped when i2 < 0 && !bAllPoints
 *     or P3D2c.z < 0 (float); camera-frame points R * Xw + t in float; Huber delta = sqrtf(th2); edges in feature order;
 *   * i2 < 0: the e21 "observation" is the NORMALISED (x, y) of P3D2c compared against pixels (such edges end as outliers);
 *   * g2o's Levenberg-Marquardt (optimization_algorithm_levenberg.cpp:61-169) with numeric Jacobians (delta 1e-9, central
 *     differences), sums in edge order, the 7 x 7 system by Eigen::LDLT; the phase-1 inlier test reads the errors of the last
 *     EVALUATED trial (a failed last trial is popped without recomputing them);
 *   * KannalaBrandt8::project(Vector3d) calls atan2f / sqrtf in float (its numeric Jacobian is quantised the same way) and cos / sin of
 *     a double: glibc's, bit for bit (csrc/libm_f32.h, csrc/libm_f64.h).
 * Rig keyframes: the reference reads pKF1->mvKeysUn[i] for every i, out of bounds for i >= NLeft on a KB8 rig; pass feature i's own
 * row (mvKeysRight[i - NLeft]) as DESIGN.md section 6 decides for SearchByProjection(Frame, KeyFrame). */
int morb_optimize_sim3_batch(morb_optimizer*, int nprob, int cap, const int* d_count, const uint8_t* d_entry, const float* d_Xw1,
                             const float* d_Xw2, const int* d_i2, const float* d_obs1, const float* d_invSigma2_1, const float* d_obs2,
                             const float* d_invSigma2_2, const float* d_T1w, const float* d_T2w, const float* d_cam1, const float* d_cam2,
                             const float* d_th2, const uint8_t* d_fixScale, int bAllPoints, double* d_S12, uint8_t* d_keep, int* d_nIn,
                             int* d_stats, void* stream);

/* Sim3Solver (src/Sim3Solver.cc, include/Sim3Solver.h): the constructor, SetRansacParameters, both iterate overloads and find, for
 * nprob problems at once, one workgroup each, asynchronous on `stream` (NULL = the handle's own).  Stateless apart from the
 * per-problem state record: every call recomputes the constructor and SetRansacParameters (cheap) and runs iterate(nIterations, ...)
 * from state.iterations on, so one entry serves find() (nIterations = maxIterations), LoopClosing's chunked
 * `while (!bConverge && !bNoMore) iterate(20, ...)` (LoopClosing.cc:705-722) and one call with the whole budget.
 * Per problem (DEVICE array of records): */
typedef struct morb_sim3_solver_params {
  float T1w[12], T2w[12];   /* pKF1 / pKF2 GetRotation() row-major + GetTranslation() (:65-68); X3Dc2 always uses pKF2's pose */
  float cam1[9], cam2[9];   /* kind (0 Pinhole, 1 KannalaBrandt8) + the 8 parameters of pKF1->mpCamera / pKF2->mpCamera */
  double probability;       /* SetRansacParameters(probability, minInliers, maxIterations) (:122-146) */
  int minInliers;           /* >= 3 in every use of the reference; with fewer, N < 3 returns as N < minInliers does (sampling 3 of
                               fewer than 3 is undefined in the reference) */
  int maxIterations;
  int fixScale;             /* bFixScale: ms12i = 1 */
  int n;                    /* mN1 = vpMatched12.size() (<= cap) */
} morb_sim3_solver_params;

/* In / out, one per problem.  Zero it before the first call (the constructor's mnIterations = mnBestInliers = 0); the kernel
 * reads iterations, bestInliers and the best* fields and writes every field. */
typedef struct morb_sim3_solver_state {
  int N;             /* correspondences kept by the constructor (:76-112) */
  int budget;        /* mRansacMaxIts after SetRansacParameters (:133-143) */
  int iterations;    /* mnIterations: iterations done over all calls so far */
  int bestInliers;   /* mnBestInliers */
  int converged;     /* this call's bConverge (:246-253): an iteration had more than minInliers inliers */
  int noMore;        /* this call's bNoMore: N < minInliers (:223-226), or the budget is spent without convergence (:259) */
  int nInliers;      /* this call's nInliers: the inliers of the converged hypothesis, else 0 */
  int convergedAt;   /* global index of the converged iteration, -1 */
  float bestT12[16]; /* mBestT12 row-major (GetEstimatedTransformation) */
  float bestR[9];    /* mBestRotation row-major (GetEstimatedRotation) */
  float bestt[3];    /* mBestTranslation */
  float bestScale;   /* mBestScale */
  float sim3[16];    /* this call's return value of iterate(.., bConverge): mBestT12 on convergence, else bestSim3 = mBestT12 when an
                        iteration of THIS call reached the best count, else identity (the reference leaves bestSim3 uninitialised
                        there).  The other iterate overload and find() return identity unless converged. */
} morb_sim3_solver_state;

/* Per KF1 feature i < params.n, arrays [nprob][cap]:
 *   d_entry  bit 0 vpMatched12[i] != NULL, bit 1 pMP1 = pKF1->GetMapPointMatches()[i] != NULL, bit 2 pMP1->isBad(), bit 3 pMP2->isBad(),
 *            bit 4 get<0>(pMP1->GetIndexInKeyFrame(pKF1)) < 0, bit 5 get<0>(pMP2->GetIndexInKeyFrame(pKFm)) < 0 (:76-93);
 *   d_Xw1 / d_Xw2 [..][3] GetWorldPos() of pMP1 / pMP2;
 *   d_sigma2_1 = pKF1->mvLevelSigma2[octave of mvKeysUn[indexKF1]], d_sigma2_2 = pKFm->mvLevelSigma2[octave of pKFm->mvKeysUn[indexKF2]],
 *            pKFm = vpKeyFrameMatchedMP[i] (pKF2 when the vector is empty); thresholds (size_t)(9.210 * sigma2) (:98-99).
 * d_rand [nprob][randCap]: the rand() values of DUtils::Random::RandomInt, three per iteration, iteration g (global, from 0) reading
 * d_rand[p][3g .. 3g+2]; a call stops at iteration randCap / 3.  Outputs: d_state; d_inliers [nprob][cap] = vbInliers (all zero
 * unless converged; indexed by KF1 feature); d_hypInliers (optional) [nprob][hypCap] = the inlier count of global iteration g for
 * every g this call evaluates (entries of iterations not evaluated are left as they are: pre-fill them with -1).
 * Every iteration restates the reference in float: sampling, ComputeSim3 (Horn's closed form; the eigenvector of N by an FP64
 * cyclic Jacobi instead of Eigen::EigenSolver: DESIGN.md section 6), CheckInliers with both cameras; iterate's running best uses >=
 * and it returns at the first iteration with more than minInliers inliers. */
int morb_sim3_solver_batch(morb_optimizer*, int nprob, int cap, const morb_sim3_solver_params* d_params, const uint8_t* d_entry,
                           const float* d_Xw1, const float* d_Xw2, const float* d_sigma2_1, const float* d_sigma2_2, int nIterations,
                           const int* d_rand, int randCap, morb_sim3_solver_state* d_state, uint8_t* d_inliers, int* d_hypInliers,
                           int hypCap, void* stream);

/* MLPnPsolver (src/MLPnPsolver.cpp, include/MLPnPsolver.h): the constructor, SetRansacParameters and iterate, for nprob problems at
 * once, one workgroup each, asynchronous on `stream` (NULL = the handle's own).  Stateless apart from the per-problem state record
 * and the best mask: every call recomputes the constructor and SetRansacParameters (cheap) and runs iterate(nIterations, ...) from
 * state.iterations on, so one entry serves Tracking::Relocalization's round-robin `iterate(5, ...)` (Tracking.cc:3405-3432) and one
 * call with the whole budget.  Per problem (DEVICE array of records): */
typedef struct morb_mlpnp_solver_params {
  float cam[9];        /* kind (0 Pinhole, 1 KannalaBrandt8) + the 8 parameters of F.mpCamera (:56): unproject in the constructor
                          (:78), project in CheckInliers (:276) */
  double probability;  /* SetRansacParameters(probability, minInliers, maxIterations, minSet, epsilon, th2) (:225-260); Tracking
                          passes (0.99, 10, 300, 6, 0.5, 5.991) */
  int minInliers;      /* raised to int(N * epsilon) and to minSet (:237-242) */
  int maxIterations;   /* the budget is ceil(log(1 - p) / log(1 - eps^3)) clipped to [1, maxIterations] (:248-255) */
  int minSet;          /* correspondences per hypothesis, 6 .. 16; a value outside runs no iteration and reports budget = 0,
                          noMore = 1 (a device-side field cannot fail the call: the Python and C++ fronts, which hold the host
                          copy, return MORB_ERR_INVALID's error before the launch) */
  float epsilon;       /* raised to (float)minInliers / N (:244-245) */
  float th2;           /* mvMaxError[i] = sigma2[i] * th2 in float (:257-259) */
  int n;               /* vpMapPointMatches.size() (<= cap) */
} morb_mlpnp_solver_params;

/* In / out, one per problem.  Zero it before the first call (the constructor's mnIterations = mnBestInliers = 0); the kernel reads
 * iterations, bestInliers and bestTcw and writes every field. */
typedef struct morb_mlpnp_solver_state {
  int N;            /* correspondences kept by the constructor (:66-94) */
  int minInliers;   /* mRansacMinInliers after SetRansacParameters (:237-242) */
  int budget;       /* mRansacMaxIts after SetRansacParameters (:255) */
  int iterations;   /* mnIterations: iterations done over all calls so far */
  int bestInliers;  /* mnBestInliers */
  int ok;           /* this call's return value of iterate (:199, :218) */
  int noMore;       /* this call's bNoMore: N < minInliers (:106-110), or the budget is spent (:205-207), also beside ok = 1 of the
                       post-loop branch; not set by a call that returns from Refine() */
  int nInliers;     /* this call's nInliers: mnRefinedInliers (:191), mnBestInliers of the post-loop branch (:210), else 0 */
  int refined;      /* 1: Tcw is mRefinedTcw (:198); 0: mBestTcw (:217) or none */
  int returnedAt;   /* global index of the iteration whose Refine() succeeded, else -1 */
  float bestTcw[16];/* mBestTcw row-major (:181-183): the double pose of the best iteration rounded to float */
  float Tcw[16];    /* this call's Tout: identity unless ok */
} morb_mlpnp_solver_state;

/* Per feature i < params.n, arrays [nprob][cap]:
 *   d_entry  bit 0 vpMapPointMatches[i] != NULL, bit 1 pMP->isBad(), bit 2 i >= F.mvKeysUn.size() (:67-71); a feature is kept iff
 *            bit 0 is set and bits 1, 2 are clear;
 *   d_uv [..][2] F.mvKeysUn[i].pt (mvP2D, float; the bearing vector is unproject(pt) / z in float, NOT normalised, :74-81);
 *   d_sigma2 = F.mvLevelSigma2[kp.octave] (:75);  d_Xw [..][3] pMP->GetWorldPos() (:84-86).
 * d_rand [nprob][randCap]: the rand() values of DUtils::Random::RandomInt (:130), minSet per iteration (six with the reference's
 * default), iteration g (global, from 0) reading d_rand[p][minSet * g .. minSet * g + minSet - 1]; a call stops at iteration
 * randCap / minSet.  nIterations is iterate's first argument: the loop condition (:115) is an OR, so a call runs to the end of the
 * budget or nIterations iterations, whichever comes later.
 * d_bestInliers [nprob][cap], in / out: mvbBestInliers by feature; the kernel clears it while state.bestInliers == 0, so a zeroed
 * state needs nothing else.  Outputs: d_state; d_inliers [nprob][cap] = vbInliers by feature (all zero unless ok); d_hypInliers
 * (optional) [nprob][hypCap] = mnInliersi of global iteration g for every g this call evaluates (entries of iterations not
 * evaluated are left as they are: pre-fill them with -1).
 * computePose (:356-658) runs in FP64 with the project's own routines where the reference calls Eigen (cyclic Jacobi for the
 * 12 x 12 / 9 x 9 / 3 x 3 symmetric eigenproblems, the 3 x 3 SVD built on it, a 6 x 6 LDL^T, a hand-derived Gauss-Newton Jacobian:
 * DESIGN.md section 6, "MLPnPsolver"); CheckInliers (:262-293) rounds R X + t to float and projects in float, error2 < maxError. */
int morb_mlpnp_solver_batch(morb_optimizer*, int nprob, int cap, const morb_mlpnp_solver_params* d_params, const uint8_t* d_entry,
                            const float* d_uv, const float* d_sigma2, const float* d_Xw, int nIterations, const int* d_rand, int randCap,
                            morb_mlpnp_solver_state* d_state, uint8_t* d_bestInliers, uint8_t* d_inliers, int* d_hypInliers, int hypCap,
                            void* stream);

/* bool TwoViewReconstruction::Reconstruct(vKeys1, vKeys2, vMatches12, T21, vP3D, vbTriangulated), src/TwoViewReconstruction.cc:41-130 with
 * everything it calls and GeometricTools::Triangulate (src/GeometricTools.cc:48-72): what Pinhole::ReconstructWithTwoViews
 * (src/CameraModels/Pinhole.cpp:85-98) runs for Tracking::MonocularInitialization (src/Tracking.cc:2326).  nprob problems, one workgroup
 * each, asynchronous on the stream.  Problem p = (image d_img1[p], image d_img2[p]) of a keypoint pool [nimg][cap] with its counts, as
 * the matcher entries take them: d_kpsUn holds mvKeysUn (undistorted; a KannalaBrandt8 caller undistorts first), and
 * d_matches12 [nprob][cap] is vnMatches12 as the SearchForInitialization entry above writes it (an entry outside [0, count of image 2)
 * is no match).  d_K4 [nprob][4] = fx fy cx cy of toK_(), d_sigma [nprob] = mSigma (1.0 in the reference).  maxIterations = the
 * constructor's iterations (200).  d_rand [nprob][randCap]: the rand() values of DUtils::Random::RandomInt (:87), eight per iteration,
 * iteration-major.  Outputs: d_ok [nprob] the return value; d_T21 [nprob][12] R21 row-major then t21 (zero unless ok);
 * d_P3D [nprob][cap][3] and d_triangulated [nprob][cap] by frame-1 keypoint: the winning hypothesis' vP3D / vbTriangulated on BOTH
 * paths (ReconstructH of this fork never assigns vP3D, :712-718), zero everywhere else, beyond the count and whenever ok is 0;
 * d_stats [nprob][16] and d_fstats [nprob][29]: rows indexed by the enums TwoViewStat / TwoViewFStat of include/morb/two_view_math.h
 * (N, model, best iterations, inlier count, nGood and parallax of every motion hypothesis, the chosen one, why it failed; SH SF RH, the
 * best H21 and F21).  Optional (NULL to skip): d_inliersH / d_inliersF [nprob][cap] the best masks BY MATCH (entry k = the k-th match in
 * frame-1 order), d_hypScores [nprob][2][maxIterations] the score of every iteration, H then F.
 * Fewer than eight matches (undefined in the reference): no iteration, ok 0, model 0.  MORB_ERR_INVALID before any launch for
 * maxIterations below 1, randCap below 8 * maxIterations or cap below 1.  The SVDs are the project's own FP64 Jacobi routines, the score
 * sums the reference's sequential float sums ("TwoViewReconstruction"). */
int morb_two_view_reconstruction_batch(morb_optimizer*, int nprob, int cap, const int* d_img1, const int* d_img2, const int* d_count,
                                       const morb_keypoint* d_kpsUn, const int* d_matches12, const float* d_K4, const float* d_sigma,
                                       int maxIterations, const int* d_rand, int randCap, int* d_ok, float* d_T21, float* d_P3D,
                                       uint8_t* d_triangulated, int* d_stats, float* d_fstats, uint8_t* d_inliersH, uint8_t* d_inliersF,
                                       float* d_hypScores, void* stream);

/* The numeric rest of void Tracking::CreateInitialMapMonocular(), src/Tracking.cc:2345-2430, behind the two entries above:
 * Optimizer::GlobalBundleAdjustemnt(map, 20) -> BundleAdjustment over the two new keyframes and their points (src/Optimizer.cc:47-362),
 * KeyFrame::ComputeSceneMedianDepth(2) of the first keyframe (src/KeyFrame.cc:796-826), the reset test (:2407-2408), the rescaling of the
 * baseline and of every point (:2416-2429) and MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:464-519).  nprob problems, one workgroup
 * each, one launch, asynchronous on the stream, no host synchronisation.  Inputs as the two entries above leave them: the keypoint pool
 * [nimg][cap] with its counts (mvKeysUn), d_matches12 [nprob][cap], d_ok [nprob], d_T21 [nprob][12] (R21 row-major, then t21), d_P3D
 * [nprob][cap][3], d_triangulated [nprob][cap].  The map points of a problem are the frame-1 keypoints i with d_matches12[i] in
 * [0, count of image 2) and d_triangulated[i] set (:2318-2323).  P (HOST) gives mvInvLevelSigma2 = 1 / levelSigma2[octave] and
 * mvScaleFactors; cam8 (HOST, fx fy cx cy k0..k3; NULL = the pinhole camera of P) with kb8 != 0 for KannalaBrandt8 (cam8 required).
 * Graph (:113-268): keyframe 1 fixed at the identity, keyframe 2 free from d_T21, two EdgeSE3ProjectXYZ per point on mvKeysUn[idx].pt,
 * Huber delta (float) sqrt(5.99) when robust != 0.  g2o Levenberg-Marquardt over BlockSolver_6_3 in FP64, nIterations outer iterations (20
 * at the call site), lambda from the largest diagonal entry of the pose and of every point.  d_stop (optional, NULL = none): [nprob]
 * bytes in device memory, pbStopFlag per problem, read at entry and at every iteration and trial.  After the solve: median = the depth
 * of rank (n - 1) / 2 in keyframe 1, in float; invMedianDepth = depthScale / median (depthScale 1; 4 for IMU-monocular; 0 = do not
 * scale: the state BundleAdjustment itself leaves); reset when median < 0 or fewer than minTracked (50) points, nothing scaled then.
 * Outputs: d_status [nprob] (0 = ok was 0 and nothing ran, 1 = ok, else the reset reasons as bits: 2 = negative median or no point,
 * 4 = too few points); d_Tcw2 [nprob][12]; by frame-1 keypoint and zero elsewhere d_mpPos [nprob][cap][3], d_mpNormal [nprob][cap][3],
 * d_mpDist [nprob][cap][2] (mfMaxDistance, mfMinDistance; observers keyframe 1 and 2, reference keyframe 2, level = the octave of its
 * keypoint) and d_hasMP [nprob][cap]; d_stats [nprob][4] = points, outer iterations, LM trials, stop seen; d_chi2 [nprob][2] = first
 * and last active chi2; d_median [nprob].  A problem whose ok is 0 gets zero rows.  MORB_ERR_INVALID before any launch for cap < 1,
 * nIterations < 0, nprob < 0 or a NULL required pointer.  Points are bounded by cap alone: their records live in LDS up to cap 512, in
 * a grow-only workspace of the handle beyond ("Initial map"). */
int morb_create_initial_map_monocular_batch(morb_optimizer*, const morb_frame_params* P, const float* cam8, int kb8, int nprob, int cap,
                                            const int* d_img1, const int* d_img2, const int* d_count, const morb_keypoint* d_kpsUn,
                                            const int* d_matches12, const int* d_ok, const float* d_T21, const float* d_P3D,
                                            const uint8_t* d_triangulated, int nIterations, int robust, float depthScale, int minTracked,
                                            const unsigned char* d_stop, int* d_status, float* d_Tcw2, float* d_mpPos, float* d_mpNormal,
                                            float* d_mpDist, uint8_t* d_hasMP, int* d_stats, double* d_chi2, float* d_median, void* stream);

/* ---- visual-inertial tracking and mapping ----
 * IMU::Preintegrated as plain data (include/ImuTypes.h:154-263): 3 x 3 blocks row-major, C = the 15 x 15 covariance
 * row-major, b = the bias the measurements were integrated with in IMU::Bias order (bax bay baz bwx bwy bwz),
 * nga / ngaWalk = the diagonals of IMU::Calib::Cov / CovWalk (gyro x3, acc x3; ImuTypes.cc:375-388). */
typedef struct {
  float dT;
  float dR[9], dV[3], dP[3];
  float JRg[9], JVg[9], JVa[9], JPg[9], JPa[9];
  float C[225];
  float b[6];
  float nga[6], ngaWalk[6];
  float avgA[3], avgW[3];
} morb_imu_preintegrated;

/* IMU::Preintegrated::Initialize + IntegrateNewMeasurement over each measurement sequence (ImuTypes.cc:152-170, :191-247;
 * what Tracking::PreintegrateIMU feeds it, Tracking.cc:1705-1790) for nseq sequences at once.  DEVICE pointers:
 * sequence s owns the measurements [d_start[s], d_start[s+1]) of d_acc / d_gyro ([.][3]) and d_dt; d_bias [nseq][6].
 * ngaDiag6 / walkDiag6 are HOST pointers. */
int morb_imu_preintegrate_batch(morb_optimizer*, int nseq, const int* d_start, const float* d_acc, const float* d_gyro,
                                const float* d_dt, const float* d_bias, const float* ngaDiag6, const float* walkDiag6,
                                morb_imu_preintegrated* d_out, void* stream);

/* static int Optimizer::PoseInertialOptimizationLastKeyFrame(Frame* pFrame, bool bRecInit)  Optimizer.h:127-128,
 * Optimizer.cc:4391-4757, for nframes frames at once (DEVICE pointers, frame f at offset f*cap; same per-feature arrays
 * as morb_pose_optimization_batch plus d_close[i] != 0 <=> mvpMapPoints[i]->mTrackDepth < 10).  States are Rwb (9,
 * row-major), twb, velocity, gyro bias, acc bias = 21 floats: d_kfState = pFrame->mpLastKeyFrame (fixed vertices),
 * d_state in/out = the frame (GetImuRotation / GetImuPosition / GetVelocity / mImuBias -> SetImuPoseVelocity, mImuBias).
 * Tbc12 (HOST) = mImuCalib.mTbc rotation (9) + translation (3); d_pre[f] = pFrame->mpImuPreintegrated.
 * d_nInliers[f] = the return value; d_prior (optional) [nframes][246] doubles = pFrame->mpcpi (ConstraintPoseImu): the
 * 21 state values in FP64 followed by the 15 x 15 H (after the constructor's eigenvalue clamp), row-major.  One pinhole camera; the _fisheye forms below take a KannalaBrandt8 rig. */
int morb_pose_inertial_optimization_last_keyframe_batch(morb_optimizer*, int nframes, int cap, const int* d_count,
                                                        const uint8_t* d_hasMP, const float* d_obs, const float* d_invSigma2,
                                                        const float* d_Xw, const uint8_t* d_close, float fx, float fy, float cx,
                                                        float cy, float bf, const float* Tbc12, const float* d_kfState,
                                                        const morb_imu_preintegrated* d_pre, int bRecInit, float* d_state,
                                                        uint8_t* d_outlier, int* d_nInliers, double* d_prior, void* stream);

/* static int Optimizer::PoseInertialOptimizationLastFrame(Frame* pFrame, bool bRecInit)  Optimizer.h:125-126,
 * Optimizer.cc:4761-5161: the frame and the previous frame (d_prevState, free) are optimised together, tied by
 * EdgeInertial(d_preFrame = pFrame->mpImuPreintegratedFrame), the bias random walks (information from d_preKF =
 * pFrame->mpImuPreintegrated) and EdgePriorPoseImu(d_prevPrior = pFp->mpcpi, [nframes][246] doubles as produced by either
 * function).  d_prior (optional) = the frame's new mpcpi after Optimizer::Marginalize(H, 0, 14).  Other arguments as above. */
int morb_pose_inertial_optimization_last_frame_batch(morb_optimizer*, int nframes, int cap, const int* d_count,
                                                     const uint8_t* d_hasMP, const float* d_obs, const float* d_invSigma2,
                                                     const float* d_Xw, const uint8_t* d_close, float fx, float fy, float cx, float cy,
                                                     float bf, const float* Tbc12, const float* d_prevState,
                                                     const morb_imu_preintegrated* d_preFrame, const morb_imu_preintegrated* d_preKF,
                                                     const double* d_prevPrior, int bRecInit, float* d_state, uint8_t* d_outlier,
                                                     int* d_nInliers, double* d_prior, void* stream);

/* static void Optimizer::LocalInertialBA(KeyFrame* pKF, bool* pbStopFlag, Map* pMap, int&, int&, int&, int&, bool bLarge,
 * bool bRecInit)  Optimizer.h:71-74, Optimizer.cc:2324-2897, on the graph the reference assembles at :2337-2768, flattened
 * (HOST pointers).  nKF keyframes with states of 21 floats (Rwb row-major, twb, velocity, gyro bias, acc bias);
 * kfKind[k]: 0 = temporal optimizable keyframe (vpOptimizableKFs), 1 = the fixed keyframe before the window (its IMU
 * state enters the last inertial link), 2 = fixed keyframe that only observes points (lFixedKeyFrames).  nMP points
 * (mpClose[j] != 0 <=> mTrackDepth < 10), nE observations (eObs = x, y, uRight; uRight < 0 = EdgeMono, else EdgeStereo).
 * nI inertial links: iKF1 = mPrevKF, iKF2 = the keyframe owning iPre[i] (mpImuPreintegrated); iRobust[i] != 0 and
 * iInfoScale[i] = 1e-2 on the link to the fixed keyframe (and iRobust on all links when bRecInit) as at :2553-2563; each
 * link also carries EdgeGyroRW / EdgeAccRW.  bLarge selects 4 iterations / lambda 1e-2 instead of 10 / 1.
 * Outputs: kfState21 (optimizable keyframes) and mpPos in place, eraseFlag[e] = 1 where the reference erases the
 * observation (:2773-2826), stats3 = {outer LM iterations, LM trials, ok} with ok = 0 for "FAIL LOCAL-INERTIAL BA"
 * (nothing written back).  One pinhole camera; morb_local_inertial_ba_fisheye for a KB8 rig. */
int morb_local_inertial_ba(morb_optimizer*, int nKF, float* kfState21, const uint8_t* kfKind, int nMP, float* mpPos,
                           const uint8_t* mpClose, int nE, const int* eKF, const int* eMP, const float* eObs, const float* eInvSigma2,
                           int nI, const int* iKF1, const int* iKF2, const morb_imu_preintegrated* iPre, const uint8_t* iRobust,
                           const float* iInfoScale, float fx, float fy, float cx, float cy, float bf, const float* Tbc12, int bLarge,
                           uint8_t* eraseFlag, int* stats3);

/* The three inertial optimisers on a fisheye rig (pFrame->mpCamera2 / pKFi->mpCamera2: Optimizer.cc:4453-4528, :2722-2754;
 * ImuCamPose with two cameras, G2oTypes.cc:96-113).  rig28 (HOST) = left KannalaBrandt8 parameters (8), right ones (8), the
 * rotation (9, row-major) and translation (3) of Frame::GetRelativePoseTrl().  Every observation is monocular: features
 * [0, d_nLeft[f]) / edges with eRight[e] == 0 on the left camera (EdgeMonoOnlyPose(Xw, 0) / EdgeMono(0), mvKeys), the rest on
 * the right camera (cam_idx 1, mvKeysRight); d_obs / eObs = (x, y, unused).  Other arguments as the pinhole forms. */
int morb_pose_inertial_optimization_last_keyframe_fisheye_batch(morb_optimizer*, int nframes, int cap, const int* d_count, const int* d_nLeft,
                                                                const uint8_t* d_hasMP, const float* d_obs, const float* d_invSigma2,
                                                                const float* d_Xw, const uint8_t* d_close, const float* rig28,
                                                                const float* Tbc12, const float* d_kfState,
                                                                const morb_imu_preintegrated* d_pre, int bRecInit, float* d_state,
                                                                uint8_t* d_outlier, int* d_nInliers, double* d_prior, void* stream);
int morb_pose_inertial_optimization_last_frame_fisheye_batch(morb_optimizer*, int nframes, int cap, const int* d_count, const int* d_nLeft,
                                                             const uint8_t* d_hasMP, const float* d_obs, const float* d_invSigma2,
                                                             const float* d_Xw, const uint8_t* d_close, const float* rig28, const float* Tbc12,
                                                             const float* d_prevState, const morb_imu_preintegrated* d_preFrame,
                                                             const morb_imu_preintegrated* d_preKF, const double* d_prevPrior, int bRecInit,
                                                             float* d_state, uint8_t* d_outlier, int* d_nInliers, double* d_prior,
                                                             void* stream);
int morb_local_inertial_ba_fisheye(morb_optimizer*, int nKF, float* kfState21, const uint8_t* kfKind, int nMP, float* mpPos,
                                   const uint8_t* mpClose, int nE, const int* eKF, const int* eMP, const float* eObs, const uint8_t* eRight,
                                   const float* eInvSigma2, int nI, const int* iKF1, const int* iKF2, const morb_imu_preintegrated* iPre,
                                   const uint8_t* iRobust, const float* iInfoScale, const float* rig28, const float* Tbc12, int bLarge,
                                   uint8_t* eraseFlag, int* stats3);

/* void static Optimizer::InertialOptimization in its three overloads (Optimizer.h:103-112), the steps behind LocalMapping::InitializeIMU /
 * ScaleRefinement (LocalMapping.cc:1205, :1391) and the bias re-estimation after a map merge (LoopClosing.cc:1902), for nprob problems at
 * once (DEVICE pointers).  Problem p owns the keyframes [d_kfStart[p], d_kfStart[p+1]) in temporal order; cap (HOST) bounds the keyframes of
 * any one problem (workspace and LDS / global tier; above 4096: MORB_ERR_CAPACITY before any launch).  d_kfState21[k] = Rwb (9, row-major),
 * twb, velocity, gyro bias, acc bias; poses are read only.  d_hasLink[k] != 0: keyframe k carries an EdgeInertialGS (G2oTypes.cc:587-727)
 * to keyframe k - 1 of its problem with d_pre[k] = its mpImuPreintegrated (the conditions of Optimizer.cc:3077-3078); a problem's first
 * keyframe never has one, a zero in the middle is a broken chain (isBad() or no mPrevKF).  mode (HOST): 0 = InertialOptimization(pMap, Rwg,
 * scale, bg, ba, bMono, covInertial, bFixedVel, bGauss, priorG, priorA) (Optimizer.cc:2979-3156), 1 = (pMap, bg, ba, priorG, priorA)
 * (:3158-3314), 2 = (pMap, Rwg, scale) (:3316-3428).  d_flags[p]: bit 0 bMono, bit 1 bFixedVel (mode 0 only); d_prior2[p] = {priorG, priorA}.
 * d_global16[p] (FP64, in / out) = Rwg (9, row-major), scale, bg (3), ba (3): on entry bg / ba are the initial estimate of the bias vertices
 * (vpKFs.front()'s bias in every mode; in mode 2 the fixed bias of every link).  Modes 0 and 1 write every keyframe's velocity
 * (Vw.cast<float>()) and bias fields (SetNewBias(b)), d_reintegrate[k] = 1 where the reference calls Reintegrate() (float norm of the old gyro
 * bias minus bg.cast<float>() above 0.01, on a keyframe with a link), bg, ba and, in mode 0, Rwg and scale; mode 1 works with Rwg = I and
 * scale = 1 whatever the array holds and leaves those ten values untouched; mode 2 writes Rwg and scale only.  d_stats4[p] = {outer
 * iterations, LM trials (0 for Gauss-Newton), ok, links}; d_chi2[p] = activeRobustChi2 before and after.  A problem with fewer than two
 * keyframes or without a link: ok = 0, nothing else written.  g2o Levenberg-Marquardt (200 iterations, lambda 1e3 when priorG != 0 in mode 0
 * and always in mode 1) or, mode 2, Gauss-Newton (10 iterations, Huber delta 1 on every link) in one launch, one workgroup per problem
 * ("InertialOptimization"). */
int morb_inertial_optimization_batch(morb_optimizer*, int nprob, int cap, const int* d_kfStart, float* d_kfState21,
                                     const uint8_t* d_hasLink, const morb_imu_preintegrated* d_pre, int mode,
                                     const int* d_flags, const float* d_prior2, double* d_global16,
                                     uint8_t* d_reintegrate, int* d_stats4, double* d_chi2, void* stream);

/* static void Optimizer::LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag, Map* pMap, int& num_fixedKF,
 * int& num_OptKF, int& num_MPs, int& num_edges)  Optimizer.h:67-69, Optimizer.cc:1053-1441, on the graph the
 * reference assembles at :1058-1351, flattened (HOST pointers): nKF keyframes (local ones first or in any
 * order; kfFixed[i] != 0 for lFixedCameras and the map's initial keyframe), nMP local map points, nE
 * observations (eKF, eMP indices; eObs = (x, y, uRight); eInvSigma2).  lambdaInit100 != 0 <=>
 * pMap->IsInertial() (:1137).  stopFlag = pbStopFlag itself (a bool is one byte; NULL = none): read at entry (the graph is
 * not optimised when set, :1355) and polled at every LM iteration and trial like optimizer.setForceStopFlag does (:1142).
 * Outputs: optimised kfPose (free keyframes) and mpPos in place, eraseFlag[e] = 1 where the reference erases the
 * observation (:1366-1401), stats2 = {outer LM iterations, LM trials}. */
int morb_local_bundle_adjustment(morb_optimizer*, int nKF, float* kfPose, const uint8_t* kfFixed, int nMP, float* mpPos,
                                 int nE, const int* eKF, const int* eMP, const float* eObs, const float* eInvSigma2,
                                 float fx, float fy, float cx, float cy, float bf, int lambdaInit100,
                                 const unsigned char* stopFlag, uint8_t* eraseFlag, int* stats2);

/* The same in three steps, so that a problem can stay resident in HBM and be solved repeatedly (benchmarks) or
 * aborted from another thread: create (upload + CSR build), solve (device only, asynchronous on `stream`,
 * restarts from the uploaded initial values), results (synchronises, downloads).  morb_ba_set_stop mirrors
 * LocalMapping::InterruptBA -> mbAbortBA (LocalMapping.cc:884): the flag lives in pinned host memory mapped into the
 * device, so setting it makes no HIP call, may come from any thread while a solve runs, and is seen at the top of the
 * next outer iteration / LM trial like in g2o (sparse_optimizer.cpp:376, optimization_algorithm_levenberg.cpp:149). */
typedef struct morb_ba_problem morb_ba_problem;
int morb_ba_problem_create(morb_optimizer*, morb_ba_problem** out, int nKF, const float* kfPose, const uint8_t* kfFixed,
                           int nMP, const float* mpPos, int nE, const int* eKF, const int* eMP, const float* eObs,
                           const float* eInvSigma2, float fx, float fy, float cx, float cy, float bf,
                           int lambdaInit100);

/* The same for a KannalaBrandt8 stereo rig (pKFi->mpCamera2 != NULL, Optimizer.cc:1244-1351): every observation is an
 * EdgeSE3ProjectXYZ with the left camera (eRight[e] == 0; mvuRight < 0 on such rigs, so there are no stereo edges) or
 * an EdgeSE3ProjectXYZToBody with the right camera behind mTrl (eRight[e] != 0, observation = mvKeysRight[rightIndex
 * - NLeft].pt).  eObs2 = [nE][2]; camL8 / camR8 = fx fy cx cy k0..k3; Trl7 = GetRelativePoseTrl() as quaternion xyzw +
 * translation.  Erase rule: chi2 > 5.991 || !isDepthPositive() for both kinds (:1366-1390). */
int morb_ba_problem_create_fisheye(morb_optimizer* o, morb_ba_problem** out, int nKF, const float* kfPose, const uint8_t* kfFixed,
                                   int nMP, const float* mpPos, int nE, const int* eKF, const int* eMP, const float* eObs2,
                                   const uint8_t* eRight, const float* eInvSigma2, const float* camL8, const float* camR8,
                                   const float* Trl7, int lambdaInit100);
int morb_local_bundle_adjustment_fisheye(morb_optimizer* o, int nKF, float* kfPose, const uint8_t* kfFixed, int nMP, float* mpPos,
                                         int nE, const int* eKF, const int* eMP, const float* eObs2, const uint8_t* eRight,
                                         const float* eInvSigma2, const float* camL8, const float* camR8, const float* Trl7,
                                         int lambdaInit100, const unsigned char* stopFlag, uint8_t* eraseFlag, int* stats2);
void morb_ba_problem_destroy(morb_ba_problem*);
int morb_ba_set_stop(morb_ba_problem*, int stop);
/* mode 0 (default): one launch per LM phase over the whole GPU, accept / reject decided on the device; mode 1: the whole LM loop
 * inside ONE persistent workgroup (for many small problems). */
int morb_ba_set_mode(morb_ba_problem*, int mode);
/* Mode 0 BLOCKS the calling host thread until the last LM decision: it queues trial after trial on `stream`, one trial ahead of the
 * decisions, and watches two words in mapped host memory (forwarding the caller's stop flag meanwhile); MORB_ERR_HIP if the stream
 * reports a fault while it waits.  The kernels queued behind the last decision are empty; results are read with morb_ba_results
 * (which synchronises).  Mode 1 only enqueues one launch. */
int morb_ba_solve(morb_ba_problem*, void* stream);
int morb_ba_results(morb_ba_problem*, float* kfPose, float* mpPos, uint8_t* eraseFlag, int* stats2);
/* Measurement hook (bench.py's LocalBA roofline entry; not a reference method): times the FP64-MFMA Schur product of block_solver.hpp:
 * 354-480 on the operands the last morb_ba_solve left behind.  flops = MFMA flops issued per launch, usefulFlops = the sparse form's. */
int morb_ba_schur_profile(morb_ba_problem*, int iters, float* msPerLaunch, double* flops, double* usefulFlops);

/* void static Optimizer::LocalBundleAdjustment(KeyFrame* pMainKF, vector<KeyFrame*> vpAdjustKF, vector<KeyFrame*> vpFixedKF,
 * bool* pbStopFlag)  Optimizer.h:115-118, Optimizer.cc:3430-3851: the "welding" bundle adjustment LoopClosing::MergeLocal runs over the
 * current window and the matched map's window (LoopClosing.cc:1652), on the graph the reference assembles at :3459-3648, flattened (HOST
 * pointers) like morb_local_bundle_adjustment: kfFixed[i] != 0 for vpFixedKF, 0 for vpAdjustKF (the map's initial keyframe is not special
 * here); one edge per observation, eObs = (x, y, uRight) with uRight < 0 for a monocular observation (EdgeSE3ProjectXYZ, else
 * EdgeStereoSE3ProjectXYZ); information eInvSigma2 * I; Huber deltas (float)sqrt(5.99) and (float)sqrt(7.815) (:3547-3548); no user lambda.
 * stopFlag = pbStopFlag itself (one byte; NULL = none): set at entry (:3650) the call returns MORB_OK with stats6 all zero and nothing else
 * written; it is polled at every LM iteration and trial (:3452), and set after round 1 (:3658) it skips round 2.  Round 1 is optimize(5)
 * with the Huber kernels; then every edge with chi2() > 5.991 (7.815 stereo) or a non-positive depth goes to level 1, every edge loses its
 * kernel, and round 2 is initializeOptimization(0); optimize(10) over the level-0 edges (:3662-3698) with the Levenberg-Marquardt state of
 * a fresh start.  Outputs: kfPose of the free keyframes and mpPos in place (:3784-3850; fixed keyframes keep their bytes), eraseFlag[e] = 1
 * where the reference erases the observation (:3705-3739: the same test, on the chi2() the edge holds — for a level-1 edge the value of the
 * end of round 1 — and on the depth at the final estimate), levelFlag[e] = 1 for the edges excluded from round 2 (may be NULL), stats6 =
 * {round-1 outer iterations, round-1 trials, round-2 outer iterations, round-2 trials, edges put on level 1, rounds run (0: the flag was set
 * at entry, else 1 or 2)}.  Both rounds, the classification between them and the flags are one queue of launches with the LM control on the
 * device ("Welding bundle adjustment"). */
int morb_merge_bundle_adjustment(morb_optimizer*, int nKF, float* kfPose, const uint8_t* kfFixed, int nMP, float* mpPos,
                                 int nE, const int* eKF, const int* eMP, const float* eObs, const float* eInvSigma2,
                                 float fx, float fy, float cx, float cy, float bf, const uint8_t* stopFlag,
                                 uint8_t* eraseFlag, uint8_t* levelFlag, int* stats6);
/* The same on a KannalaBrandt8 rig: mvuRight < 0 there, so every edge is an EdgeSE3ProjectXYZ with pKF->mpCamera, the left camera
 * (:3582-3602; this function makes no right-camera "ToBody" edge).  eObs2 = [nE][2]; camL8 = fx fy cx cy k0..k3. */
int morb_merge_bundle_adjustment_fisheye(morb_optimizer*, int nKF, float* kfPose, const uint8_t* kfFixed, int nMP, float* mpPos,
                                         int nE, const int* eKF, const int* eMP, const float* eObs2, const float* eInvSigma2,
                                         const float* camL8, const uint8_t* stopFlag, uint8_t* eraseFlag, uint8_t* levelFlag,
                                         int* stats6);

/* void static Optimizer::MergeInertialBA(KeyFrame* pCurrKF, KeyFrame* pMergeKF, bool* pbStopFlag, Map* pMap,
 * LoopClosing::KeyFrameAndPose& corrPoses)  Optimizer.h:110-112, Optimizer.cc:3853-4389: the welding bundle adjustment of an inertial map
 * merge (LoopClosing::MergeLocal at LoopClosing.cc:1649-1650 for IMU_MONOCULAR / IMU_STEREO / IMU_RGBD, MergeLocal2 at :2099), on the graph
 * the reference assembles at :3985-4272, flattened (HOST pointers) like morb_local_inertial_ba: nKF keyframes with states of 21 floats (Rwb
 * row-major, twb, velocity, gyro bias, acc bias); kfKind[k]: 0 = free with 15 unknowns (vpOptimizableKFs, and vpOptimizableCovKFs[0], the
 * head of the current map's chain, whose velocity and bias vertices hang on the first inertial edge), 1 = fixed with an IMU state that
 * enters a link (lFixedKeyFrames, behind the merge map's chain), 2 = fixed keyframe that only observes points, 3 = free in the pose only,
 * 6 unknowns (the further vpOptimizableCovKFs, and keyframes with !bImu: their velocity and bias vertices carry no edge, so g2o leaves them
 * out of the active set).  nMP points, nE observations (eObs = x, y, uRight; uRight < 0 = EdgeMono(0), else EdgeStereo; information
 * eInvSigma2 * I, Huber deltas (float)sqrt(5.991) / (float)sqrt(7.815)).  nI inertial links: iKF1 = mPrevKF, iKF2 = the keyframe owning
 * iPre[i]; every link is an EdgeInertial with Huber delta sqrt(16.92) and its information unscaled (:4115-4128) plus EdgeGyroRW / EdgeAccRW
 * (:4130-4146); the two temporal chains are told apart by nothing but their indices.  A link between two
 * keyframes of kind 1 is taken as g2o takes an edge between fixed vertices: it moves nothing and adds its robust chi2, a constant, to every sum.  A link with an endpoint of kind 2 or 3, an index out
 * of range, a NULL array (pbStopFlag may be NULL) or an empty graph: MORB_ERR_INVALID before any launch, nothing written.
 * setUserLambdaInit(1e3), optimize(8) (:3995, :4280); no "FAIL" test.  pbStopFlag is the caller's flag itself (one byte): set at entry
 * (:4276) the call returns MORB_OK with stats3 = {0, 0, 0} and nothing else written; it is polled at every LM iteration and trial (:4274).
 * Outputs: kfState21 in place — all 21 floats of kind 0, the pose (Rwb, twb) of kind 3 whose velocity and bias floats keep their bytes, as
 * do kinds 1 and 2 entirely; mpPos in place; eraseFlag[e] = 1 where the reference erases the observation (:4287-4310: chi2() > 5.991f,
 * stereo 7.815f — no depth test, no mTrackDepth rule); stats3 = {outer LM iterations, LM trials, ran}.  The reduced system has 15 n15 +
 * 6 n6 unknowns ("MergeInertialBA").  Left with the caller: the window selection (:3856-3983), SetNewBias on the
 * preintegrations before the call (:4092) and on the keyframes after it, UpdateNormalAndDepth (:4385) and corrPoses (:4333-4335, :4359-4361)
 * — include/morb/Optimizer_reference.h does all four on the reference's types. */
int morb_merge_inertial_ba(morb_optimizer*, int nKF, float* kfState21, const uint8_t* kfKind, int nMP, float* mpPos,
                           int nE, const int* eKF, const int* eMP, const float* eObs, const float* eInvSigma2,
                           int nI, const int* iKF1, const int* iKF2, const morb_imu_preintegrated* iPre,
                           float fx, float fy, float cx, float cy, float bf, const float* Tbc12,
                           const uint8_t* pbStopFlag, uint8_t* eraseFlag, int* stats3);
/* The same on a KannalaBrandt8 rig (rig28 as morb_local_inertial_ba_fisheye takes it): every edge is an EdgeMono(0) on the left camera —
 * this function creates no right-camera edge (:4224-4244); eObs = (x, y, unused). */
int morb_merge_inertial_ba_fisheye(morb_optimizer*, int nKF, float* kfState21, const uint8_t* kfKind, int nMP, float* mpPos,
                                   int nE, const int* eKF, const int* eMP, const float* eObs, const float* eInvSigma2,
                                   int nI, const int* iKF1, const int* iKF2, const morb_imu_preintegrated* iPre,
                                   const float* rig28, const float* Tbc12,
                                   const uint8_t* pbStopFlag, uint8_t* eraseFlag, int* stats3);

/* void static Optimizer::OptimizeEssentialGraph(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF, const LoopClosing::KeyFrameAndPose&
 * NonCorrectedSim3, const LoopClosing::KeyFrameAndPose& CorrectedSim3, const map<KeyFrame*, set<KeyFrame*>>& LoopConnections, const bool&
 * bFixScale)  Optimizer.h:76-81, Optimizer.cc:1443-1735: the Sim3 pose graph LoopClosing::CorrectLoop optimises behind the fusion
 * (LoopClosing.cc:1206-1208), on the graph the reference assembles at :1477-1682, flattened (HOST pointers); the graph of the second overload
 * (:1737-2063, many fixed vertices) has the same form.  nKF vertices: kfSim3[k] = qx qy qz qw tx ty tz s, the g2o::Sim3 estimate
 * (CorrectedSim3's entry, or the keyframe's pose with s = 1, :1485-1495), in and out; kfFlags[k] bit 0 = setFixed(true) (:1497), bit 1 =
 * _fix_scale (:1501).  nE EdgeSim3 in insertion order: setVertex(0, eI), setVertex(1, eJ), measurement eSji[e] in the same eight doubles;
 * information = identity, no robust kernel (:1537-1546).  Several edges may join one pair; an edge between two fixed vertices is a
 * constant of chi2.  setUserLambdaInit(1e-16) (:1458), optimize(20) (:1686) with g2o's Levenberg-Marquardt over numeric Jacobians
 * (EdgeSim3 has no linearizeOplus); H + lambda I is solved exactly by a block-sparse LDL^T over the envelope of the 7 x 7 block rows in
 * the order of the vertices given (pass them by ascending mnId: the spanning tree and the covisibility edges then form a band, the loop
 * edges a few long rows; DESIGN.md section 6, "Essential graph").  A vertex without an edge is not in g2o's active set: it is not in
 * the system and keeps its bytes, as a fixed one does.  A free component with no path to a fixed vertex is gauge-free: it is neither
 * detected nor repaired.  The point correction of :1707-1731 runs on the device behind the solve: mpRef[m] = the vertex of
 * mnCorrectedReference or of the reference keyframe (:1714-1720), -1 = skip (a bad point); mpPos[m] becomes
 * correctedSwr.map(Srw.map(P)) in FP64, then float, Srw being the vertex's value at entry.  nMP = 0 is allowed (mpPos, mpRef may be NULL).
 * stats4 = {outer LM iterations, LM trials, vertices in the system, envelope blocks}; chi2 = the active chi2 before and after.
 * MORB_ERR_INVALID: a NULL array, an index out of range, eI == eJ, a non-finite estimate or measurement or a scale <= 0;
 * MORB_ERR_CAPACITY: the envelope exceeds what the handle may grow to (2^22 blocks); both before any launch, nothing written.  No free
 * vertex has an edge (nE = 0 included; eI, eJ, eSji may then be NULL): MORB_OK, nothing written, stats4 and chi2 zero.  Left with the caller: the edge list itself (:1514-1682), SetPose
 * with t / s (:1691-1705), UpdateNormalAndDepth and IncreaseChangeIndex (:1730-1734). */
int morb_optimize_essential_graph(morb_optimizer*, int nKF, double* kfSim3, const uint8_t* kfFlags, int nE, const int* eI,
                                  const int* eJ, const double* eSji, int nMP, float* mpPos, const int* mpRef, int* stats4,
                                  double* chi2);
/* void static Optimizer::OptimizeEssentialGraph(KeyFrame* pCurKF, vector<KeyFrame*>& vpFixedKFs, vector<KeyFrame*>& vpFixedCorrectedKFs,
 * vector<KeyFrame*>& vpNonFixedKFs, vector<MapPoint*>& vpNonCorrectedMPs)  Optimizer.h:83-87, Optimizer.cc:1737-2063: the Sim3 pose graph
 * LoopClosing::MergeLocal optimises behind the welding bundle adjustment on every non-monocular sensor (LoopClosing.cc:1747-1749), flattened
 * (HOST pointers).  nKF vertices, the keyframes of the three lists that are not bad, in ascending mnId (the order of elimination).
 * kfLists[k]: bit 0 = vpFixedKFs (fixed, _fix_scale, vpGoodPose; :1783-1808), bit 1 = vpFixedCorrectedKFs (fixed, good and bad, vScw from
 * mTcwBefMerge; :1813-1843), bit 2 = vpNonFixedKFs (free with a free scale, vpBadPose, vScw = the pose; :1845-1874).  Legal values: 1, 2, 4,
 * and 6 for a keyframe of both the window and the non-fixed list, which keeps the vertex of the window (sIdKF, :1850) and still gets the
 * tail.  kfTcw / kfTwc / kfTcwBefMerge / kfTwcBefMerge = GetPose(), GetPoseInverse(), mTcwBefMerge, mTwcBefMerge of every vertex, 7 floats
 * each (unit quaternion xyzw and translation, as morb_merge_bundle_adjustment takes a pose), in and out.  nC candidate edges in the
 * reference's insertion order (:1888-1999), chosen by topology alone: setVertex(0, cI), setVertex(1, cJ); a keyframe of two lists is
 * visited twice there and gives its candidates twice.  The entry applies the rule of :1907-1913 itself — an edge exists where both ends
 * are good or both are bad — and reports it in cKept[c] (1 = the edge exists).  Its measurement is Sjw * Swi with the reference's quirks:
 * Swi = vScw[i]^-1 only where i is bad, so for a keyframe of vpFixedKFs it is the default g2o::Sim3(), the identity; Sjw =
 * (vCorrectedSwc[j])^-1 where both are good, else vScw[j]; correctedSwi is never used.  An edge between two fixed vertices moves nothing and
 * is a constant of chi2, which g2o's stop rule sees.  On the device: the float poses go to FP64 through Sophus' normalising cast, the
 * measurements are formed, then setUserLambdaInit(1e-16) (:1767), optimize(20) (:2010) by the solver of morb_optimize_essential_graph
 * unchanged, then the tail of :2015-2062: every vertex with bit 2 gets kfTcwBefMerge / kfTwcBefMerge = the bytes of kfTcw / kfTwc at entry,
 * kfTcw = SE3d(q, t / s).cast<float>() and kfTwc = its inverse as SE3f::inverse computes it in float (SetPose); every other vertex keeps
 * the bytes of all four.  A vertex without an edge is not in the system; with bit 2 its pose still makes the float -> double -> float
 * round trip.  mpRef[m] = the vertex of the point's reference keyframe, -1 = skip (a bad point, a reference outside the lists); a point
 * whose reference has bit 1 or bit 2 becomes (Twr * TwrBefMerge^-1) * P in float — the SE3f product first, then the point — with Twr and
 * TwrBefMerge as they stand behind the tail (for a vertex of bit 1 alone: kfTwc and kfTwcBefMerge as given, LoopClosing.cc:1544-1546);
 * a point whose reference is in vpFixedKFs keeps its bytes (:2059-2061).  Quaternions are normalised as Eigen's four-wide sum does it,
 * (x^2 + z^2) + (y^2 + w^2).  nMP = 0 is allowed (mpPos, mpRef may be NULL), and nC = 0 (cI, cJ, cKept may be NULL).  stats4 and chi2 as
 * morb_optimize_essential_graph gives them.  No free vertex has an edge: the solve is skipped, stats4 and chi2 are zero, the tail still
 * runs.  MORB_ERR_INVALID: a NULL array, an index out of range, cI == cJ, a non-finite pose or a zero quaternion (the poses before the merge
 * are read, and checked, for vertices with bit 1 only), a value of kfLists other than 1, 2, 4, 6 (the reference would add one vertex id
 * twice); MORB_ERR_CAPACITY: the envelope exceeds what the handle may grow to (2^22 blocks); both before any launch, nothing written.  One
 * upload and one download, on the handle's stream.  Left with the caller: the candidate list (:1888-1999), the map's mutex, SetPose,
 * SetWorldPos, UpdateNormalAndDepth and the EraseObservation loop of :2038-2048. */
int morb_optimize_essential_graph_merge(morb_optimizer*, int nKF, const uint8_t* kfLists, float* kfTcw, float* kfTwc,
                                        float* kfTcwBefMerge, float* kfTwcBefMerge, int nC, const int* cI, const int* cJ,
                                        uint8_t* cKept, int nMP, float* mpPos, const int* mpRef, int* stats4, double* chi2);
/* acos(d[i]) and log(s[i]) as g2o::Sim3::log (types/sim3.h:151, :181) gets them inside morb_optimize_essential_graph: the device
 * library's, for the tests that measure them against the host libm (HOST pointers, n > 0). */
int morb_sim3_log_libm(morb_optimizer*, int n, const double* d, const double* s, double* acosOut, double* logOut);

/* void static Optimizer::OptimizeEssentialGraph4DoF(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF, const LoopClosing::KeyFrameAndPose&
 * NonCorrectedSim3, const LoopClosing::KeyFrameAndPose& CorrectedSim3, const map<KeyFrame*, set<KeyFrame*>>& LoopConnections)
 * Optimizer.h:89-94, Optimizer.cc:5163-5472: the pose graph LoopClosing::CorrectLoop optimises in an inertial map whose IMU is
 * initialised (LoopClosing.cc:1200-1203), on the graph the reference assembles at :5194-5426, flattened (HOST pointers).  nKF vertices
 * VertexPose4DoF (G2oTypes.h:155-189): kfPose[k] = Rcw[0] row-major and tcw[0], in and out; kfBody[k] = Rwb row-major and twb at entry.
 * The two are given independently, as the reference's constructors fill them (from a keyframe's float members, or from
 * CorrectedSim3.inverse()): the first computeError reads kfPose as given, and the camera pose follows the body state from the first
 * accepted update on (UpdateW, G2oTypes.cc:218-248, with its counter of five updates).  The unknowns are (yaw, tx, ty, tz) of the body
 * in the world.  kfFixed[k] != 0 = setFixed(true) (:5216).  Tcb12 = mImuCalib.mTcb, one calibration for the map.  nE Edge4DoF
 * (G2oTypes.h:816-842) in insertion order: setVertex(0, eI), setVertex(1, eJ), eTij[e] = dRij row-major and dtij; information
 * diag(1e3, 1e3, 1, 1, 1, 1), no robust kernel (:5231-5234).  Several edges may join one pair; an edge between two fixed vertices is a
 * constant of chi2.  optimize(20) (:5430) with g2o's Levenberg-Marquardt over numeric Jacobians; no setUserLambdaInit: the first lambda is
 * 1e-5 * the largest diagonal entry of the first system.  H + lambda I is solved exactly by a block LDL^T over the envelope of the 4 x 4
 * block rows in the order of the vertices given (pass them by ascending mnId; DESIGN.md section 6, "4-DoF pose graph").  A vertex without
 * an edge is not in g2o's active set: it is not in the system and keeps its bytes, as a fixed one does.  The point correction of
 * :5451-5470 runs on the device behind the solve: mpRef[m] = the vertex of the reference keyframe, -1 = skip (a bad point); mpPos[m]
 * becomes correctedSwr.map(Srw.map(P)) in FP64, then float, with Srw = kfScw[ref] = qx qy qz qw tx ty tz s, the g2o::Sim3 vScw at entry
 * (it keeps the scale of a CorrectedSim3 entry), and correctedSwr the inverse of (Rcw, tcw, 1) of the result.  nMP = 0 is allowed
 * (mpPos, mpRef, kfScw may be NULL).  stats4 = {outer LM iterations, LM trials, vertices in the system, envelope blocks}; chi2 = the active
 * chi2 before and after.  MORB_ERR_INVALID: a NULL array, an index out of range, eI == eJ, a non-finite value, a scale <= 0 in kfScw;
 * MORB_ERR_CAPACITY: the envelope exceeds what the handle may grow to (2^22 blocks); both before any launch, nothing written.  No free
 * vertex has an edge (nE = 0 included; eI, eJ, eTij may then be NULL): MORB_OK, nothing written, stats4 and chi2 zero.  Left with the
 * caller: the edge list itself (:5236-5426), SetPose (:5435-5448), UpdateNormalAndDepth and IncreaseChangeIndex (:5468-5471). */
int morb_optimize_essential_graph_4dof(morb_optimizer*, int nKF, double* kfPose, const double* kfBody, const uint8_t* kfFixed,
                                       const float* Tcb12, int nE, const int* eI, const int* eJ, const double* eTij, int nMP,
                                       float* mpPos, const int* mpRef, const double* kfScw, int* stats4, double* chi2);

/* void static Optimizer::BundleAdjustment(const vector<KeyFrame*>& vpKF, const vector<MapPoint*>& vpMP, int nIterations, bool* pbStopFlag,
 * const unsigned long nLoopKF, const bool bRobust)  Optimizer.h:49-52, Optimizer.cc:56-362: the whole-map bundle adjustment
 * Optimizer::GlobalBundleAdjustemnt (:47-54) hands every keyframe and point of the map to, which LoopClosing::RunGlobalBundleAdjustment starts
 * behind a corrected loop (LoopClosing.cc:2302: 10 iterations, bRobust = false), on the graph the reference assembles at :113-268, flattened
 * (HOST pointers) like morb_local_bundle_adjustment.  nKF keyframes, kfPose[k] = quaternion xyzw and t (7 floats), in and out; kfFixed[k] !=
 * 0 stands for setFixed(pKF->mnId == pMap->GetInitKFid()) (:121) — the caller may fix more.  nMP points, mpPos in and out.  nE edges in
 * insertion order (:144-260: by point, within a point by observing keyframe, the left observation before the right one): eKF, eMP, eObs =
 * (x, y, uRight), information eInvSigma2 * I; uRight < 0 gives EdgeSE3ProjectXYZ (:155-183), else EdgeStereoSE3ProjectXYZ (:184-221).
 * Several edges may share one (eKF, eMP) pair; they add into one Hpl block in edge order.  nIterations in 1 .. 100 is optimize(nIterations)
 * (:273); there is no setUserLambdaInit: the first lambda is 1e-5 * the largest diagonal entry of the first system over the pose and the
 * point blocks (g2o's computeLambdaInit).  bRobust != 0: Huber kernels with delta (float)sqrt(5.99) on the monocular and (float)sqrt(7.815)
 * on the stereo edges (:126-127, :171-175, :204-208 — 5.99, not 5.991); 0: those edges carry no kernel (the loop-closing case).  stopFlag =
 * pbStopFlag itself (one byte; NULL = none), polled at every LM iteration and trial (:78); set at entry the call returns MORB_OK with stats4
 * and chi2 zero and nothing else written.  H + lambda I of the reduced camera system is solved exactly by a block LDL^T over the envelope of
 * the 6 x 6 block rows in the order of the keyframes given: pass them by ascending mnId, so that covisible keyframes are neighbours and the
 * envelope is a band with a few long rows where a loop was closed ("Global bundle adjustment"); the Schur complement of
 * the points is built block by block over that envelope, nothing dense in nMP x nKF is allocated.  Outputs: kfPose of the free keyframes
 * that carry an edge and mpPos of the points that carry one (:276-361); fixed keyframes, keyframes without an edge and points without an
 * edge (:262-264) keep their bytes.  stats4 = {outer LM iterations, LM trials, keyframes in the system, envelope blocks}; chi2 = the active
 * robust chi2 before and after.  This function erases no observation: the counts of :297-340 feed nothing and are left out.
 * MORB_ERR_INVALID: a NULL array, an empty graph, an index out of range, a non-finite pose, point, observation or information, nIterations
 * outside 1 .. 100; MORB_ERR_CAPACITY: the envelope exceeds what the handle may grow to (the bytes of the Sim3 pose graph's 2^22 blocks:
 * 2^22 * 49 / 36 blocks of 6 x 6), or the Schur complement has more pair contributions than an int indexes (a point seen by k free
 * keyframes gives k (k + 1) / 2); all before any launch, nothing written.  No free keyframe has an edge: MORB_OK, nothing written, stats4 and
 * chi2 zero.  Left with the caller: the graph itself (:113-268), and SetPose / SetWorldPos / UpdateNormalAndDepth or mTcwGBA / mPosGBA /
 * mnBAGlobalForKF (:276-361). */
int morb_bundle_adjustment(morb_optimizer*, int nKF, float* kfPose, const uint8_t* kfFixed, int nMP, float* mpPos,
                           int nE, const int* eKF, const int* eMP, const float* eObs, const float* eInvSigma2,
                           float fx, float fy, float cx, float cy, float bf, int nIterations, int bRobust,
                           const uint8_t* stopFlag, int* stats4, double* chi2);
/* The same on a KannalaBrandt8 stereo rig (pKF->mpCamera2 != NULL), with the arrays of morb_local_bundle_adjustment_fisheye: eObs2 =
 * [nE][2]; eRight[e] == 0 is an EdgeSE3ProjectXYZ with the left camera (mvuRight < 0 on such rigs: no stereo edge), eRight[e] != 0 an
 * EdgeSE3ProjectXYZToBody with the right camera behind mTrl (:223-259), usually behind the left edge of the same keyframe and point.  A
 * ToBody edge always carries Huber's kernel with delta (float)sqrt(5.99), whatever bRobust says (:244-246): restated, not repaired. */
int morb_bundle_adjustment_fisheye(morb_optimizer*, int nKF, float* kfPose, const uint8_t* kfFixed, int nMP, float* mpPos,
                                   int nE, const int* eKF, const int* eMP, const float* eObs2, const uint8_t* eRight,
                                   const float* eInvSigma2, const float* camL8, const float* camR8, const float* Trl7,
                                   int nIterations, int bRobust, const uint8_t* stopFlag, int* stats4, double* chi2);

/* void static Optimizer::FullInertialBA(Map* pMap, int its, const bool bFixLocal, const unsigned long nLoopKF, bool* pbStopFlag, bool bInit,
 * float priorG, float priorA, Eigen::VectorXd* vSingVal, bool* bHess)  Optimizer.h:55-58, Optimizer.cc:364-760: the inertial whole-map
 * bundle adjustment — LoopClosing::RunGlobalBundleAdjustment at LoopClosing.cc:2305 (7 iterations, once the map's IMU is initialised) and
 * LocalMapping::InitializeIMU at LocalMapping.cc:1244-1249 (100 iterations, bInit with the priors or without) — on the graph the reference
 * assembles at :392-687, flattened (HOST pointers) like morb_merge_inertial_ba: nKF keyframes in ascending mnId (the caller's business: the
 * envelope is a band then) with states of 21 floats (Rwb row-major, twb, velocity, gyro bias, acc bias), in and out; kfKind[k]: 0 = free with
 * 15 unknowns (a bImu keyframe that enters a link), 1 = fixed with an IMU state that enters a link (bFixLocal), 2 = fixed keyframe that only
 * observes points, 3 = free in the pose only, 6 unknowns (!bImu keyframes and bImu keyframes without a link: their velocity and bias
 * vertices carry no edge, so g2o leaves them out of the active set).  nMP points, nE observations ordered by point, then keyframe, the left
 * observation before the right one, as morb_bundle_adjustment takes them (eObs = x, y, uRight; uRight < 0 = EdgeMono(0), else EdgeStereo;
 * information eInvSigma2 * I; every one under Huber with delta (float)sqrt(5.991) / (float)sqrt(7.815), :556-557).  nI links: iKF1 = mPrevKF,
 * iKF2 = the keyframe owning iPre[i] (after SetNewBias(mPrevKF->GetImuBias()), :455): an EdgeInertial under Huber with delta sqrt(16.92) and
 * its information unscaled (:493-505), and with !bInit EdgeGyroRW / EdgeAccRW with the inverted C blocks and no kernel (:507-528).  bInit:
 * ONE gyro and one accelerometer bias for the map (:427-436), bias6 = gyro then accelerometer, in and out (read and written only then, and
 * non-NULL then; the caller takes it from the last keyframe, pIncKF): every EdgeInertial hangs on them, there are no random-walk edges, a
 * kind-0 keyframe owns 9 unknowns, and EdgePriorGyro / EdgePriorAcc at zero with information priorG I / priorA I are added (:535-554).  The
 * priors' error is 0 - bias and their Jacobian is taken as -I, as the error demands; G2oTypes.cc:768-776 states +I.  A link between two
 * keyframes of kind 1 is a constant of the robust chi2 (with bInit it still moves the shared biases).  setUserLambdaInit(1e-5) (:384),
 * optimize(its) once (:693), its in 1 .. 100.  pbStopFlag is the caller's flag itself (one byte, NULL = none): set at entry (:689) the call
 * returns MORB_OK with stats4 and chi2 zero and nothing else written; it is polled at every LM iteration and trial (:388).
 * H + lambda I of the reduced system — 15, 9 or 6 rows per keyframe, 6 last rows for the shared biases that cover every linked keyframe — is
 * solved exactly by a block LDL^T over the envelope of its 3 x 3 block rows ("FullInertialBA"); only the six pose
 * columns of a keyframe meet a point, the Schur complement is built block by block, nothing dense in nMP x nKF or nKF x nKF is allocated.
 * Outputs: kfState21 in place — all 21 floats of kind 0 (with bInit its bias floats hold the shared value, :719-738), the pose (Rwb, twb) of
 * kind 3 whose velocity and bias floats keep their bytes, as do kinds 1 and 2 entirely and a kind-3 keyframe without an edge; mpPos of the
 * points that carry an edge; bias6; stats4 = {outer LM iterations, LM trials, scalar unknowns of the reduced system, envelope blocks of
 * 3 x 3}; chi2 = the active robust chi2 before and after.  MORB_ERR_INVALID: a NULL array, an empty graph, an index out of range, a link
 * with an endpoint of kind 2 or 3 or with iKF1 == iKF2, a keyframe of kind 0 that enters no link (pass it as kind 3), a NaN or Inf input, its
 * outside 1 .. 100; MORB_ERR_CAPACITY: the envelope exceeds what the handle may grow to (the bytes morb_bundle_adjustment allows: 2^22 * 49 /
 * 9 blocks), the Schur complement has more contributions than an int indexes, or there are 2^23 links or more; all before any launch, nothing
 * written.  No keyframe in the
 * system: MORB_OK, nothing written, stats4 and chi2 zero.  Left with the caller: the graph itself — bFixLocal and its `< 3` return
 * (:401-440), bad keyframes, maxKFid, points seen by fixed keyframes only (:683-686: pass them without edges) — SetNewBias on the
 * preintegrations, and SetPose / SetVelocity / SetNewBias / SetWorldPos / UpdateNormalAndDepth or mTcwGBA / mVwbGBA / mBiasGBA / mPosGBA /
 * mnBAGlobalForKF (:696-759).  vSingVal and bHess are never touched by the reference. */
int morb_full_inertial_ba(morb_optimizer*, int nKF, float* kfState21, const uint8_t* kfKind, int nMP, float* mpPos,
                          int nE, const int* eKF, const int* eMP, const float* eObs, const float* eInvSigma2,
                          int nI, const int* iKF1, const int* iKF2, const morb_imu_preintegrated* iPre,
                          float fx, float fy, float cx, float cy, float bf, const float* Tbc12,
                          int its, int bInit, float priorG, float priorA, float* bias6,
                          const uint8_t* pbStopFlag, int* stats4, double* chi2);
/* The same on a KannalaBrandt8 rig (rig28 as morb_local_inertial_ba_fisheye takes it): every edge is an EdgeMono, eRight[e] != 0 on the
 * right camera (EdgeMono(1), :648-679), usually behind the left edge of the same keyframe and point; eObs = (x, y, unused). */
int morb_full_inertial_ba_fisheye(morb_optimizer*, int nKF, float* kfState21, const uint8_t* kfKind, int nMP, float* mpPos,
                                  int nE, const int* eKF, const int* eMP, const float* eObs, const uint8_t* eRight,
                                  const float* eInvSigma2, int nI, const int* iKF1, const int* iKF2,
                                  const morb_imu_preintegrated* iPre, const float* rig28, const float* Tbc12,
                                  int its, int bInit, float priorG, float priorA, float* bias6,
                                  const uint8_t* pbStopFlag, int* stats4, double* chi2);

#ifdef __cplusplus
}
#endif
#endif /* MORB_HIP_H */
