/* world_class_codec.h -- the reference's feature codec on the MI355X, exported by
 * libworldclass_hip.so: mel-cepstral coding of the spectral envelope by DCT-through-FFT and 3 kHz-band coding of the
 * aperiodicity (reference include/codec.hpp:23-90, src/codec.cpp:211-325).
 *
 * The five functions of the reference keep their names, argument meaning and row-pointer tables (include/codec.hpp is the
 * drop-in header); they copy the rows to the device, run the kernels below and copy back.  The *_device variants work on
 * device-resident parameters in the packed layout of world_class_c.h (rows of fft_size/2+1 doubles, coded rows of
 * number_of_dimensions / GetNumberOfAperiodicities(fs) doubles), which is the point of the codec on a GPU: it is the
 * natural epilogue of CheapTrick / D4C and shrinks what has to cross PCIe by 10-40x.
 * No CPU fallback: without a HIP device the host-pointer functions print the error and leave their outputs untouched
 * (they are void in the reference), the device variants return WC_ERR_DEVICE.
 */
#ifndef WORLD_CLASS_CODEC_H
#define WORLD_CLASS_CODEC_H

#ifdef __cplusplus
extern "C" {
#endif

/* reference include/codec.hpp:23, src/codec.cpp:211-214: int(min(15000, fs / 2 - 3000) / 3000) */
int GetNumberOfAperiodicities(int fs);
/* reference include/codec.hpp:38-39, src/codec.cpp:216-236.  Below 12 kHz there is no band and nothing is written. */
void CodeAperiodicity(const double *const *aperiodicity, int f0_length, int fs, int fft_size, double **coded_aperiodicity);
/* reference include/codec.hpp:53-54, src/codec.cpp:238-267.  Below 12 kHz (no band) the reference's mean of zero bands is NaN, so
 * every frame counts as voiced: each row becomes 10^(v/20) of the line v from -60 dB at 0 Hz to -1e-12 dB at fs/2, and the coded
 * rows are not read.  So does this function, and wc_decode_aperiodicity_device. */
void DecodeAperiodicity(const double *const *coded_aperiodicity, int f0_length, int fs, int fft_size, double **aperiodicity);
/* reference include/codec.hpp:69-71, src/codec.cpp:269-296 */
void CodeSpectralEnvelope(const double *const *spectrogram, int f0_length, int fs, int fft_size, int number_of_dimensions,
						  double **coded_spectral_envelope);
/* reference include/codec.hpp:86-88, src/codec.cpp:298-325 */
void DecodeSpectralEnvelope(const double *const *coded_spectral_envelope, int f0_length, int fs, int fft_size,
							int number_of_dimensions, double **spectrogram);

/* device-resident batches; all return 0 or a negative WC_ERR_* code (wc_last_error() has the message).  The two spectral-envelope
 * calls return with their work complete (one synchronisation of the calling thread's stream at their end); their plan is built
 * once per (device, fs, fft_size) and kept, as for the calls on both rows below. */
int wc_code_spectral_envelope_device(int fs, int fft_size, long long n_frames, int number_of_dimensions, const double *d_sp,
									 double *d_coded);
int wc_decode_spectral_envelope_device(int fs, int fft_size, long long n_frames, int number_of_dimensions, const double *d_coded,
									   double *d_sp);
int wc_code_aperiodicity_device(int fs, int fft_size, long long n_frames, const double *d_ap, double *d_coded);  /* fs >= 12 kHz */
int wc_decode_aperiodicity_device(int fs, int fft_size, long long n_frames, const double *d_coded, double *d_ap);
/* Both decoders in one pass, the input of Synthesis from coded features: d_coded_sp (n_frames x number_of_dimensions) and
 * d_coded_ap (n_frames x GetNumberOfAperiodicities(fs)) -> d_sp, d_ap (n_frames x (fft_size/2+1) each).  fft_size 2048: one
 * wavefront per frame with the transform in registers; 512, 1024, 4096: the two kernels above.  fft_size 512..4096,
 * 1 <= number_of_dimensions <= fft_size/2, fs of at least 12 kHz.  Stream-ordered at every size (enqueues only, after the first call at a
 * new (fs, fft_size)). */
int wc_decode_features_device(int fs, int fft_size, long long n_frames, int number_of_dimensions, const double *d_coded_sp,
                              const double *d_coded_ap, double *d_sp, double *d_ap);
/* The decoder with the demo's formant shift inside (world_class_io.h): wc_decode_features_device followed by
 * wc_modify_parameters_frames_device(fs, fft_size, n_frames, NULL, d_sp, NULL, d_spectral_ratio) -- d_spectral_ratio holds one
 * ratio per frame with that call's per-frame rules (0 = leave the row, an invalid value = a row of NaN); the aperiodicity rows
 * are not modified.  fft_size 2048: the stretch happens inside the one-wavefront kernel, on the log envelope it holds before its
 * exp (no extra pass over the rows, no log, no second exp; d_sp within 1e-12 relative of the two calls); 512, 1024, 4096: the
 * two calls, bit for bit.  d_spectral_ratio == NULL: wc_decode_features_device, bit for bit. */
int wc_decode_features_modified_device(int fs, int fft_size, long long n_frames, int number_of_dimensions,
                                       const double *d_coded_sp, const double *d_coded_ap, const double *d_spectral_ratio,
                                       double *d_sp, double *d_ap);
/* Both coders in one pass: d_sp, d_ap (n_frames x (fft_size/2+1)) -> d_coded_sp (n_frames x number_of_dimensions),
 * d_coded_ap (n_frames x GetNumberOfAperiodicities(fs)).  d_ap and d_coded_ap may both be NULL (sp only; then any fs).
 * fft_size 2048, 4096: one wavefront per frame with the transform in registers; 512, 1024: the kernels of the two single coders.
 * Either way the plan is built once per (device, fs, fft_size) and kept, so a call only enqueues on the calling thread's stream
 * (wc_set_stream) and never waits for the device, and a frame's coded rows depend on that frame alone, bit for bit.  Within
 * 1e-11 of the reference like the single coders, not bit-identical to them at fft_size 2048 / 4096 (another order of operations).
 * Refused with WC_ERR_INVALID, outputs untouched: another fft_size, number_of_dimensions outside 1 .. fft_size/4+1, aperiodicity
 * below 12 kHz, exactly one of d_ap / d_coded_ap NULL, NULL sp arrays with n_frames > 0, n_frames < 0 or above 2^32-1. */
int wc_code_features_device(int fs, int fft_size, long long n_frames, int number_of_dimensions, const double *d_sp,
                            const double *d_ap, double *d_coded_sp, double *d_coded_ap);

#ifdef __cplusplus
}
#endif
#endif /* WORLD_CLASS_CODEC_H */
