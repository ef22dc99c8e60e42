// The host half that the batch calls of the model features share (wc_features.hip, which defines it, and wc_gv.hip): the shape
// checks, the utterance descriptors' way to the device, and the hand-over of Device::features_scratch from stream to stream.
#pragma once
#include "wc_internal.hpp"

namespace wc {

struct FtUtt {
	long long f_off;  // first frame in the packed arrays
	int n, pad;
};

// the shape arguments every call shares, refused with WC_ERR_INVALID under the name `who`; *total: the frames of the batch
int ft_check_shape(const char *who, int n_utt, const int *lengths, int nd, int n_ap, int orders, int orders_min, int format, long long *total);
// the descriptors on the device and the scratch reserved, both handed to stream s
int ft_prepare(Device *dev, hipStream_t s, int n_utt, const int *lengths, size_t scratch_bytes, const FtUtt **d_utt);
// behind the call's last kernel: the next call on another stream waits for it
int ft_finish(Device *dev, hipStream_t s);

}  // namespace wc
