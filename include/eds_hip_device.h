/* eds_hip_device.h — inputs of a tracker handle (include/eds_hip.h) that already live in device memory: event frames, event
 * slices, keyframe points and inverse depths are read where they are by kernels on the handle's stream, instead of being
 * narrowed or packed on the host into pinned staging as the eds_trk_set_* / eds_trk_build_* calls do.  What a slot holds
 * afterwards is what the host call leaves there from the same values, bit for bit.  The symbols are exported by libeds_hip.so.
 *
 * Conventions are those of eds_hip.h: plain pointers and sizes, EDS_OK or a negative eds_status, eds_last_error() for the text.
 *  - EDS_ERR_INVALID: bad slot ranges, counts, strides or dtypes, a null or misaligned source, and every source pointer that
 *    eds_dev_check_range refuses.  Arguments are looked at in that order: a bad range returns before any pointer is examined.
 *  - EDS_ERR_STATE: a batch in flight (eds_trk_optimize_batch without eds_trk_sync); eds_dev_set_idepths on a slot without keyframe.
 *  Nothing is queued and nothing changes on either of these.
 *  - EDS_ERR_HIP: the runtime refused a copy or a launch, possibly with part of the work queued.  The slots of the range then no
 *    longer count as holding what the call was to give them (event frame; keyframe for eds_dev_set_keyframes and eds_dev_set_idepths): set them again.
 *
 * Pointers.  Arguments named d_* are read by kernels.  Every ingest call runs eds_dev_check_range on each of them, over exactly
 * the extent it will read (strides included), before it queues anything: a pageable host pointer handed to a kernel is a fault
 * for the whole device on a system without XNACK, and the check turns that mistake into an error code.  All other pointers
 * (offsets, N, K, norms) are host memory, read or written before the call returns.
 *
 * Ordering.  The ingest calls queue their kernels on the handle's stream and return; only eds_dev_build_event_frames waits (it
 * returns the norms).  The handle's stream is non-blocking, so it is NOT ordered against the null stream or any other stream:
 *   eds_dev_wait_stream(h, producer)    the handle's stream waits for everything queued on `producer` so far;
 *   ... ingest calls ...
 *   eds_dev_signal_stream(h, consumer)  `consumer` waits for everything queued on the handle's stream so far.
 * A source buffer may be overwritten or freed only after eds_dev_signal_stream towards the stream that does so, or eds_trk_sync.
 * Neither call waits on the host.  A stream argument is a hipStream_t; NULL is the null stream and needs the calls like any other.
 */
#ifndef EDS_HIP_DEVICE_H_
#define EDS_HIP_DEVICE_H_

#include <stddef.h>
#include <stdint.h>

#include "eds_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EDS_HIP_DEVICE_ABI_VERSION 1
int eds_dev_abi_version(void);

/* EDS_OK only when [p, p + bytes) lies inside ONE allocation that a kernel on `device` may read: device memory of that device
 * (an interior pointer is fine) or mapped pinned host memory.  Everything else — NULL, pageable host memory, another device's
 * memory, managed memory, a range that runs past its allocation — is EDS_ERR_INVALID with a message that names what the pointer
 * is.  Launches nothing. */
int eds_dev_check_range(int device, const void* p, size_t bytes);

/* Device buffers through the HIP runtime the library itself is bound to, for callers without a HIP binding of their own.
 * upload and download are synchronous (they return when the copy is done) and ordered against nothing else. */
int eds_dev_malloc(int device, size_t bytes, void** d_ptr);
int eds_dev_free(void* d_ptr);
int eds_dev_upload(void* d_dst, const void* h_src, size_t bytes);
int eds_dev_download(void* h_dst, const void* d_src, size_t bytes);

int eds_dev_wait_stream(eds_trk* h, void* producer_stream);
int eds_dev_signal_stream(eds_trk* h, void* consumer_stream);

/* eds_trk_set_event_frames[_f32] from device memory: slot first + b receives the H x W frame that starts at element
 * b * frame_stride of d_frames, rows row_stride elements apart (0 = dense: row_stride = W, frame_stride = H * W; otherwise
 * row_stride >= W and frame_stride >= (H - 1) * row_stride + W).  dtype: EDS_IMG_F32 or EDS_IMG_F64; fp64 is narrowed
 * round-to-nearest-even, denormals kept, overflow to +-inf.  d_frames must be aligned to its element size.  One launch. */
int eds_dev_set_event_frames(eds_trk* h, int first, int count, int dtype, const void* d_frames, int64_t frame_stride, int64_t row_stride);

/* eds_trk_build_event_frame_batch with the three event arrays in device memory: slice b is events offsets[b] .. offsets[b + 1] - 1
 * (offsets: host, count + 1 ints).  The vote reads the events in place.  norms (host, count doubles) may be NULL. */
int eds_dev_build_event_frames(eds_trk* h, int first_slot, int count, const int* offsets, const uint16_t* d_x, const uint16_t* d_y,
                               const uint8_t* d_polarity, int level, double blur_sigma, int use_exp_weights, double* norms);

/* eds_trk_set_keyframe for slots first .. first + count - 1 in one call.  N (host, count ints): points per slot, 1 .. max_points.
 * Point i of alignment b is element b * stride + i of every array (stride >= max N): d_norm_xy and d_grad_xy hold (x, y) pairs,
 * d_idp and d_w one double each.  K (host): count x {fx, fy, cx, cy}.  The Gram matrices are refreshed on the device; the call
 * does not wait for them. */
int eds_dev_set_keyframes(eds_trk* h, int first, int count, const int* N, const double* d_norm_xy, const double* d_grad_xy,
                          const double* d_idp, const double* d_w, int64_t stride, const double* K);

/* eds_trk_set_idepth_strided for slots first .. first + count - 1: the inverse depth of point i of alignment b is
 * d_idp[(b * stride + i) * elem_stride] (elem_stride >= 1: doubles between consecutive points, e.g. 4 for DepthPoints' N x 4). */
int eds_dev_set_idepths(eds_trk* h, int first, int count, const double* d_idp, int64_t stride, int elem_stride);

#ifdef __cplusplus
}
#endif
#endif /* EDS_HIP_DEVICE_H_ */
