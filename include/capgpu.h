/* capgpu.h - C ABI of libcapgpu.so: the MI355X (gfx950) replacement for the two
 * primitives that dominate CAP's PLONK prove() path, and for the prover that
 * schedules them.
 *
 * This is the drop-in boundary.  The reference (jf-cap, Rust)
 * has no FFI of its own; the seam is cut where its prover hands flat arrays to
 * arkworks.  Every entry point names the reference interface it replaces:
 *
 *   capgpu_msm_g1*        ark_ec::msm::VariableBaseMSM::multi_scalar_mul      (ark-ec 0.3.0, Cargo.lock:103-105)
 *                         via ark_poly_commit::kzg10::KZG10::commit           (Cargo.lock:208-210)
 *   capgpu_ntt_fr*        ark_poly::Radix2EvaluationDomain::{fft,ifft,
 *                         coset_fft,coset_ifft}_in_place                      (ark-poly 0.3.0, Cargo.lock:194-196)
 *   capgpu_srs_*          jf_plonk UniversalSrs / CommitKey powers_of_g       (src/proof/mod.rs:59-69, 74-109)
 *   capgpu_plonk_preprocess   PlonkKzgSnark::preprocess   (call sites src/proof/transfer.rs:133, mint.rs:76, freeze.rs:102)
 *   capgpu_plonk_prove        PlonkKzgSnark::prove::<_,_,SolidityTranscript>
 *                                                         (call sites src/proof/transfer.rs:181-186, mint.rs:113, freeze.rs:151)
 *   capgpu_plonk_verify       PlonkKzgSnark::verify::<SolidityTranscript>
 *                                                         (call sites src/proof/transfer.rs:202-207, mint.rs:132, freeze.rs:170)
 *
 * Conventions
 *   - All integers little-endian.  Field element Fr / Fq = uint64_t[4] (arkworks
 *     BigInteger256 limb order).  "Montgomery" = arkworks' in-memory Fp256 form
 *     (value * 2^256 mod p).  Scalars handed to the MSM are canonical integers
 *     (what `into_repr()` yields), exactly as arkworks' MSM takes them.
 *   - G1 affine = x, y (Montgomery), 64 bytes; the point at infinity is (0, 0)
 *     when no flag byte is present (see capgpu_srs_upload for arkworks' 72-byte
 *     struct).  G1 Jacobian = X, Y, Z (Montgomery), 96 bytes, infinity Z = 0
 *     (arkworks GroupProjective field order).
 *   - Every function returns CAPGPU_OK (0) or a negative CAPGPU_ERR_* code; it
 *     never aborts and never unwinds.  capgpu_last_error() gives a thread-local
 *     message.  The Rust shim maps non-zero to PlonkError, which prove()
 *     already maps to TxnApiError::FailedSnark (src/proof/transfer.rs:187).
 *   - Host-pointer entry points copy in/out; the caller owns its buffers for the
 *     duration of the call.  *_dev entry points take device pointers obtained
 *     from capgpu_malloc and enqueue on the library stream (capgpu_sync waits).
 *   - Thread safety: entry points may be called from any thread (rayon workers
 *     in the reference, src/utils/params_builder.rs:194-226); calls serialise
 *     on an internal lock per DEVICE CONTEXT.  One process drives as many GPUs
 *     as capgpu_init binds (see "devices" below): handles are process-wide,
 *     resident tables are replicated to a device on first use there, and
 *     host-buffer calls of threads that did not bind themselves to a device
 *     are dealt over the devices by the library.  Concurrent
 *     capgpu_plonk_prove calls can be gathered into device batches instead of
 *     queueing up: capgpu_plonk_set_coalescing.
 *   - There is no CPU fallback: without a usable gfx950 device capgpu_init
 *     fails with CAPGPU_ERR_NO_DEVICE and every other call fails with
 *     CAPGPU_ERR_NOT_INITIALISED.
 */
#ifndef CAPGPU_H
#define CAPGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CAPGPU_OK 0
#define CAPGPU_ERR_INVALID_ARG (-1)
#define CAPGPU_ERR_NO_DEVICE (-2)
#define CAPGPU_ERR_HIP (-3)
#define CAPGPU_ERR_BAD_HANDLE (-4)
#define CAPGPU_ERR_OOM (-5)
#define CAPGPU_ERR_NOT_INITIALISED (-6)
#define CAPGPU_ERR_PROOF (-7) /* prover-side failure: wrong quotient degree (unsatisfied circuit), bad sizes */
#define CAPGPU_ERR_SERIALIZATION (-8) /* malformed parameter blob: ark_serialize::SerializationError, which the
                                         reference maps to TxnApiError::DeserializationError (src/errors.rs:81-85) */
#define CAPGPU_ERR_COMM (-9) /* multi-process exchange: a peer rank failed its part, or did not arrive in time */
#define CAPGPU_ERR_BUSY (-10) /* capgpu_plonk_prove_*_async: 64 tickets outstanding; wait for one and submit again */

#define CAPGPU_NUM_WIRE_TYPES 5
#define CAPGPU_NUM_SELECTORS 13

/* Form in which the *_ex PLONK entry points take a circuit's columns (wires, selectors, sigmas):
 *   CAPGPU_INPUT_EVALS   values on the evaluation domain - n per column, row j = the value at omega^j: the finalised
 *                        circuit's tables (what the entry points without _ex take);
 *   CAPGPU_INPUT_COEFFS  polynomials in coefficient form - n coefficients per column, zero-padded: exactly what
 *                        jf-relation's `Arithmetization` trait hands the prover (`compute_wire_polynomials`,
 *                        `compute_selector_polynomials`, `compute_extended_permutation_polynomials`; the reference
 *                        holds that circuit object at src/proof/transfer.rs:181-186 and :124-155, mint.rs:76/113,
 *                        freeze.rs:102/151).  The device then skips its own interpolation and runs one forward
 *                        transform where the permutation product needs the values; a Rust binding passes the trait's
 *                        output straight through instead of undoing its interpolation on the CPU.
 *   CAPGPU_INPUT_VARS    (witnesses only) one value per VARIABLE of the circuit - what a jf-relation `PlonkCircuit` holds
 *                        (`witness: Vec<F>`); the five wire columns are that vector gathered through the circuit's wire ->
 *                        variable table (`wire_variables`), which is fixed per circuit and therefore kept by the key
 *                        (capgpu_plonk_preprocess_vars, capgpu_plonk_key_set_vars).  The gather runs on the device: a
 *                        host-resident witness costs 32 B x num_vars on the link instead of 32 B x 5 n (0.66 MB instead
 *                        of 5.24 MB for a 2-in-2-out transfer at n = 2^15); behind the gather the call is the evals form.
 * All forms give the same proof and the same keys, byte for byte. */
#define CAPGPU_INPUT_EVALS 0
#define CAPGPU_INPUT_COEFFS 1
#define CAPGPU_INPUT_VARS 2

/* ---- lifecycle ------------------------------------------------------------------------- */
/* Binds this process to the n_devices GPUs listed in device_ids (NULL / 0 selects HIP device 0): one device context
 * - stream, resident tables, scratch, lock - per id, numbered 0 .. n_devices - 1 in the order given ("slots").  The
 * reference is ONE process whose rayon threads each call prove() (src/utils/params_builder.rs:194-226); with several
 * devices bound, the library itself spreads such calls:
 *   - handles (SRS, proving keys) are process-wide; the tables behind them are copied to a device the first time it
 *     needs them (peer copy over xGMI);
 *   - capgpu_plonk_prove_batch / _prove_multi cut a host-resident batch into one part per device, proved concurrently;
 *     coalesced capgpu_plonk_prove calls (capgpu_plonk_set_coalescing) form one batch per free device; single
 *     host-buffer MSM / NTT calls go to a free device;
 *   - an SRS of >= 2^20 points (CAPGPU_SHARD_MIN_POINTS) is SHARDED by point range over the devices when it is
 *     uploaded or generated: every capgpu_msm_g1* call on it runs on all devices at once, each on the points it holds,
 *     and one exchange of the 96-byte partials (peer copies) plus n_devices - 1 additions gives the result;
 *   - *_dev entry points and capgpu_malloc work on the device of the calling thread: slot 0, or the slot the thread
 *     chose with capgpu_set_device.
 * A device may be listed once (CAPGPU_ERR_INVALID_ARG otherwise; CAPGPU_ALLOW_DUPLICATE_DEVICES=1 lifts this for tests
 * that drive the multi-device paths on one GPU).  CAPGPU_CONTEXTS_PER_DEVICE=k gives every listed device k contexts,
 * whose batches overlap on that device; the default is 4 when ONE device is bound (capgpu_device_count then reports 4:
 * a host-buffer batch is cut in two, gathered batches of coalesced calls take any free one, two parts at a time) and 1 per device otherwise.  One process per GPU (torchrun) keeps working: each process binds one device
 * and the ranks meet through capgpu_comm_* ("multi-GPU" below).  Idempotent: a second call is a no-op. */
int capgpu_init(const int* device_ids, int n_devices);
/* number of device CONTEXTS bound by capgpu_init (0 before it): the range of capgpu_set_device's slots.  NOT a GPU
 * count - one bound GPU has four contexts by default; capgpu_context_count is the same number under its proper name,
 * capgpu_physical_device_count the number of distinct HIP devices behind them. */
int capgpu_device_count(int* count_out);
int capgpu_context_count(int* count_out);
int capgpu_physical_device_count(int* count_out);
/* Binds the CALLING THREAD to context `slot` (0 .. count - 1): its *_dev calls, capgpu_malloc / memcpy / sync and its
 * host-buffer calls then all run there.  slot = -1 (the default of every thread) unbinds: device-pointer calls use slot
 * 0, host-buffer calls are dealt by the library. */
int capgpu_set_device(int slot);
/* the calling thread's binding (-1: none) and the HIP device id its device-pointer calls use */
int capgpu_get_device(int* slot_out, int* hip_device_out);
void capgpu_shutdown(void);
const char* capgpu_last_error(void);
const char* capgpu_version(void);
/* name (<= 255 chars + NUL), compute units, HBM bytes of the bound device */
int capgpu_device_info(char* name_out, int* cu_count_out, uint64_t* hbm_bytes_out);
/* Memory path between the devices of two contexts, settled by capgpu_init (hipDeviceCanAccessPeer +
 * hipDeviceEnablePeerAccess for every bound pair): *access_out = 1 direct peer access (xGMI / PCIe P2P: replication of
 * keys and SRS tables, scalar slices and partials of sharded MSMs travel device to device), 0 none (the runtime stages
 * such copies through host memory; everything still works), 2 the two contexts share one device. */
int capgpu_device_peer_info(int slot_a, int slot_b, int* access_out);
/* free / total device memory of the calling thread's device, in bytes (hipMemGetInfo) */
int capgpu_mem_info(uint64_t* free_bytes_out, uint64_t* total_bytes_out);
/* Footprint control (SURVEY 8b ownership rules: the library owns its workspace, the caller decides how much of the GPU
 * that may be).  A context's scratch - prover workspace, MSM workspace, NTT scratch, staging - grows to the largest call
 * it has served and stays (~25 GB per context after a 256-proof batch at n = 2^15; four contexts per bound device):
 *  - capgpu_trim releases the scratch, the pinned result area and the captured launch graphs of every context no call is
 *    running on; tables the caller created (SRS, proving keys, NTT domains) stay.  *bytes_released_out: device bytes
 *    given back; *contexts_busy_out: contexts skipped because a call was running on them.  The next call on a trimmed
 *    context allocates again (a hipMalloc per buffer, ~ms).
 *  - capgpu_set_memory_limit caps the scratch the library holds PER DEVICE (sum over that device's contexts; 0 = no
 *    cap, the default).  A call that would grow past it first takes the growth slack off, then trims the device's idle
 *    contexts, and then fails with CAPGPU_ERR_OOM naming the bytes it needed - the caller proves in smaller batches
 *    (scratch is proportional to the batch; what the failed call had already grown is released at its context's next
 *    entry) or raises the cap.  Scratch already held above a new cap is trimmed from
 *    idle contexts at once.  Tables are not counted.
 *  - capgpu_scratch_info: scratch bytes currently held on the calling thread's device, and the cap. */
int capgpu_trim(uint64_t* bytes_released_out, int* contexts_busy_out);
int capgpu_set_memory_limit(uint64_t scratch_bytes_per_device);
int capgpu_scratch_info(uint64_t* scratch_bytes_out, uint64_t* limit_out);
/* The allocator's counters, since capgpu_init and summed over all contexts: how often a scratch buffer or a context's
 * pinned result area GREW (one event per growth that actually allocated), the new capacities in bytes, and the wall time
 * those growths took in milliseconds - the drain of the context's streams and the release of the old buffer included.  A
 * benchmark reads them around its timed part: a non-zero difference says that an allocation (0.1 - 0.6 s for the
 * gigabytes of a large batch) landed inside it.  capgpu_plonk_reserve sizes a context ahead so that the difference is
 * zero.  With the phase trace on, every growth is also an event "scratch_grow" (a = bytes, b = microseconds).  Any pointer
 * may be NULL. */
int capgpu_scratch_stats(uint64_t* grow_events_out, uint64_t* grow_bytes_out, double* grow_ms_out);
/* Host-side phase trace (diagnostics; no reference counterpart): while on, the library timestamps the phases the kernel
 * profiler cannot see - a coalesced call's queueing, window and context wait, the host-to-device copies of a batch's
 * witnesses, the host steps between the prover's rounds, the release of the callers - into a ring of 2^20 events.
 * capgpu_trace_enable(1) starts a fresh trace, (0) stops it; capgpu_trace_dump writes one line per event
 * ("t_us thread tag a b"; tools/gpu_phase_trace.py reads it) and returns the count.  Off: one relaxed load per site. */
int capgpu_trace_enable(int on);
int capgpu_trace_dump(const char* path, uint64_t* events_out);

/* ---- device memory / stream (plumbing for callers that keep data resident) -------------- */
int capgpu_malloc(void** dev_ptr_out, size_t bytes);
int capgpu_free(void* dev_ptr);
int capgpu_memcpy_h2d(void* dev_dst, const void* host_src, size_t bytes);
int capgpu_memcpy_d2h(void* host_dst, const void* dev_src, size_t bytes);
int capgpu_sync(void);
/* waits for everything enqueued on every bound device (hipDeviceSynchronize per device): what a caller without a HIP
 * binding of its own uses where a torch program would call torch.cuda.synchronize() */
int capgpu_sync_all(void);
/* HIP runtime / driver version the PROCESS runs on (hipRuntimeGetVersion: e.g. 70226015).  The library is built against
 * /opt/rocm; a process that loaded another libamdhip64.so.7 first - PyTorch's wheel bundles its own - runs the library on
 * THAT runtime (same SONAME: the loader keeps the first).  bench.py records it: the host-witness legs differ by 3 % between
 * the two runtimes on this image. */
int capgpu_runtime_info(int* hip_runtime_version_out, int* hip_driver_version_out);
/* Device time, in milliseconds, of the work the calling thread's context executes between the two calls (HIP events on
 * its stream; _end waits for that work).  SURVEY 8d's "hipEvent around device section": bench.py times its MSM / NTT
 * legs with it.  ONE measurement per context at a time, owned by the thread that opened it: that thread may restart it
 * with a second _begin; _begin from another thread while it is open, and _end without an open measurement of the
 * calling thread, return CAPGPU_ERR_INVALID_ARG (threads that time concurrently bind different contexts:
 * capgpu_set_device). */
int capgpu_timer_begin(void);
int capgpu_timer_end(double* ms_out);
/* Run all subsequent work on the caller's hipStream_t (e.g. torch's current stream); NULL
 * restores the library's own stream.  Needs capgpu_init (CAPGPU_ERR_NOT_INITIALISED otherwise).
 *  - Scope: the stream belongs to ONE context - the calling thread's (capgpu_set_device; slot 0 for an unbound thread) -
 *    and stays until the next capgpu_set_stream on that context; the other contexts keep theirs.  Host-buffer calls of an
 *    UNBOUND thread are dealt over the contexts (capgpu_init) and so may run on a context whose stream was not switched:
 *    a caller that wants all its work on its stream binds the thread first.
 *  - Order: every launch, copy, event and wait of an entry point goes to that stream.  A *_dev call reads its device
 *    input behind whatever the caller enqueued there before, and the caller's next work on the stream sees its output;
 *    where an entry point says it does not wait for the device, that holds on the caller's stream too.  The library's
 *    helper streams (the prover's side stream and its copy stream) are joined back into the stream by events before an
 *    entry point returns.
 *  - Drain: the call waits (hipStreamSynchronize) for the stream the context is LEAVING, then switches; it does not wait
 *    for the new stream, and the helper streams hold nothing between entry points.  So work enqueued after the switch may
 *    read what work before it wrote, and tables built lazily under one stream (NTT domains, the Lagrange-form commit key,
 *    witness-check and verifier tables - each build ends with a wait of its own) are valid under the next.  The caller
 *    keeps its stream alive until it has switched away from it.
 *  - Prover: on a caller's stream a proving call neither replays captured graphs nor forks round 1 onto the side stream
 *    (the stream may carry work of the caller's); the proofs are the same bytes.  capgpu_plonk_reserve sizes for either
 *    schedule.
 *  - Tickets (capgpu_plonk_prove_*_async) are accepted.  A ticket runs on the submitter's bound context - else on any
 *    free one - and on the stream that context has when a worker starts the ticket, which need not be the one it had at
 *    submission; the proofs are the synchronous call's either way.  A caller's stream must stay alive, and should stay
 *    set, until its tickets have been waited for (capgpu_set_stream itself waits for a ticket running on the context).
 *  - Timer: capgpu_set_stream between capgpu_timer_begin and _end is allowed.  _begin's event sits in the stream that
 *    was left - drained by the switch, so it has completed - and _end's in the stream in force at _end: the time returned
 *    is the device time between those two points. */
int capgpu_set_stream(void* hip_stream);

/* ---- SRS / commit key: stays device-resident across proofs -------------------------------- */
/* bases: n affine G1 points, stride_bytes apart (64 = packed x,y; 72 = arkworks GroupAffine with
 * a trailing `infinity: bool` byte at offset 64).  coords_montgomery: 1 for arkworks memory.
 * Expands every base into its window multiples on device (one-time cost). */
int capgpu_srs_upload(const void* bases, size_t n, size_t stride_bytes, int coords_montgomery,
                      uint64_t* handle_out);
/* Synthetic SRS [tau^i] G, i < n, generated on device - the counterpart of
 * universal_setup(max_degree, rng) (src/proof/mod.rs:59-69) for benches without the Aztec file.
 * tau: canonical Fr integer. */
int capgpu_srs_generate(const uint64_t tau[4], size_t n, uint64_t* handle_out);
/* The same with the hiding powers a KZG10 setup also produces: powers_of_gamma_g = { i: [gamma tau^i] G } for degrees
 * 0 .. n (max_degree + 1), kept with the handle, written by capgpu_srs_serialize and - by degree - into the commit key of
 * every proving key preprocessed under it (capgpu_plonk_key_serialize).  The prover's commitments stay non-hiding, as
 * jf-plonk's are; the powers exist so that the stored files are what a reference-side consumer expects. */
int capgpu_srs_generate_hiding(const uint64_t tau[4], const uint64_t gamma[4], size_t n, uint64_t* handle_out);
/* bases[i] = [a + i*b] G (canonical Fr integers) - synthetic bases for the 2^24 scaling config */
int capgpu_srs_generate_affine_seq(const uint64_t a[4], const uint64_t b[4], size_t n, uint64_t* handle_out);
int capgpu_srs_size(uint64_t handle, size_t* n_out);
/* point-range shards the SRS is held in: 1, or the device count for a sharded SRS (capgpu_init) */
int capgpu_srs_shards(uint64_t handle, int* shards_out);
/* copies bases [offset, offset+n) back as packed 64-byte Montgomery affine points */
int capgpu_srs_download(uint64_t handle, size_t offset, size_t n, void* out);
int capgpu_srs_free(uint64_t handle);

/* ---- MSM: replaces VariableBaseMSM::multi_scalar_mul ------------------------------------------ */
/* out = sum_i scalars[i] * bases[offset + i];  scalars canonical 4 x u64; out Jacobian 96 B (X, Y, Z Montgomery; Z = 0:
 * infinity).  The triple is A representative of the point - like ark-ec's G1Projective it depends on the order the
 * additions were made in, which on the device varies from run to run (bucket lists are filled with atomics): compare
 * results in affine form (X / Z^2, Y / Z^3), as every caller of the reference does through into_affine(). */
int capgpu_msm_g1(uint64_t srs_handle, size_t offset, const uint64_t* scalars, size_t n, uint64_t out_xyz[12]);
/* The same commitment from a polynomial's VALUES: out = sum_{j < n} s_j [L_j(tau)] G + sum_{e < 3} s_(n+e) [tau^(n+e) -
 * tau^e] G, n = 2^log_n, L_j the Lagrange basis of the n-th roots of unity; `count` <= n + 3 scalars (the last three
 * slots are the blinders of jf-plonk's polynomials: (b0 + b1 X)(X^n - 1) for a wire, (b0 + b1 X + b2 X^2)(X^n - 1) for the
 * permutation product); scalars_montgomery != 0: arkworks' Fr memory form.  Equals capgpu_msm_g1 on the coefficients
 * ark-poly's ifft makes of the values - the form rounds 1 and 2 of the prover commit in (capgpu_plonk_set_wire_commit).
 * The Lagrange-form commit key is derived from the SRS on first use (the SRS must hold n + 3 points) and kept with it. */
int capgpu_msm_g1_lagrange(uint64_t srs_handle, uint32_t log_n, const uint64_t* scalars, size_t count,
                           int scalars_montgomery, uint64_t out_xyz[12]);
int capgpu_msm_g1_batch(uint64_t srs_handle, const size_t* offsets, const uint64_t* const* scalars,
                        const size_t* ns, int count, uint64_t* out_xyz /* count*12 */);
/* Device-resident form: d_scalars = count arrays of n scalars, scalar_stride elements apart;
 * scalars_montgomery != 0 converts from Montgomery first (what a polynomial's coefficients are);
 * d_out_xyz = count * 96 bytes on device. */
int capgpu_msm_g1_dev(uint64_t srs_handle, size_t offset, const void* d_scalars, size_t scalar_stride, size_t n,
                      int count, int scalars_montgomery, void* d_out_xyz);

/* ---- one-shot MSM: points that are used ONCE ---------------------------------------------------------------------
 * VariableBaseMSM::multi_scalar_mul(bases, scalars) as ark-ec has it (ark-ec 0.3.0 src/msm/variable_base.rs): the
 * caller's points, no handle, nothing kept.  capgpu_srs_upload expands every point into its window multiples (about 500
 * doublings and 1.3 - 2.4 KB per point) - right for a commit key that serves many proofs, more work than the MSM itself
 * for points seen once.  These entry points read the points as they are: one bucket set per window, signed digits, the
 * windows combined by Horner at the end (64 B of workspace per point, W mixed additions).  Upload an SRS when the same
 * points serve more than a handful of MSMs; call these when they serve one.
 * All of them run on the calling thread's context and its stream (capgpu_set_stream is honoured; sharding over devices
 * is not done here), take their workspace from the context's scratch (capgpu_scratch_stats counts it,
 * capgpu_set_memory_limit caps it: CAPGPU_ERR_OOM naming the bytes), check their arguments before they look for a
 * device (CAPGPU_ERR_INVALID_ARG, then CAPGPU_ERR_NOT_INITIALISED) and have no CPU fallback.  Points are taken as
 * capgpu_srs_upload takes them: not checked for being on the curve.  n = 0 gives infinity (Z = 0), count = 0 nothing.
 * A call refuses (CAPGPU_ERR_INVALID_ARG) 2^31 points or more - for the batch form: in the sum over its MSMs; up to
 * there a long input is run as point ranges of about 1.6 million points whose results are added. */
/* out = sum_i scalars[i] * bases[i]; bases as capgpu_srs_upload takes them (stride 64 / 72, coords_montgomery), scalars
 * canonical 4 x u64 (any 256-bit integer, as capgpu_msm_g1), out Jacobian 96 B.
 * Replaces VariableBaseMSM::multi_scalar_mul(&bases, &scalars) on bases that were never uploaded. */
int capgpu_msm_g1_var(const void* bases, size_t stride_bytes, int coords_montgomery, const uint64_t* scalars, size_t n,
                      uint64_t out_xyz[12]);
/* `count` independent MSMs, each over its OWN bases (packed 64-byte Montgomery affine), in one pass of launches
 * (replaces a loop of multi_scalar_mul calls, e.g. the two sides of a batched KZG check) */
int capgpu_msm_g1_var_batch(const uint64_t* const* bases, const uint64_t* const* scalars, const size_t* ns, int count,
                            uint64_t* out_xyz /* count*12 */);
/* Device-resident form, arguments in the order of capgpu_msm_g1_dev: d_bases n packed 64-byte Montgomery affine points
 * ((0,0) = infinity), never written; `count` scalar arrays over the SAME points, scalar_stride elements apart;
 * d_out_xyz count * 96 B on device.  Nothing is copied to or from the host and the call does not wait for the device. */
int capgpu_msm_g1_var_dev(const void* d_bases, const void* d_scalars, size_t scalar_stride, size_t n, int count,
                          int scalars_montgomery, void* d_out_xyz);
/* Diagnostic, as capgpu_msm_plan: "path=bucket c=13 windows=20 n_sub=65536 parts=1 sub_msms=20 ranges=1 slice=1
 * tail=horner-quad workspace_bytes=<what the launch requests from the scratch>".  Needs no device. */
int capgpu_msm_var_plan(size_t n, int count, char* buf, size_t cap);

/* ---- scalars resident with their points ("GPU g holds its bases resident and receives the matching scalar
 * slice") ------------------------------------------------------------------------------------------------------------
 * capgpu_msm_g1_dev on a sharded SRS has to scatter the caller's scalars over the devices on EVERY call (32 B x n leaving
 * one GPU: 448 MB of a 2^24-point MSM).  A caller that runs more than one MSM on the same scalars - or that can place
 * them once, ahead of time - makes them resident instead: `count` arrays over points [offset, offset + n) are cut by
 * the SRS's point ranges, each slice stored on the device that holds its points (host memory goes to each device
 * directly; device memory of the calling thread's context by one peer copy per slice).  capgpu_msm_g1_resident then
 * exchanges nothing but the 96-byte partials.  Works on an unsharded SRS too (one slice, on the calling thread's
 * context).  The set is immutable; free it with capgpu_msm_scalars_free (capgpu_shutdown frees what is left). */
int capgpu_msm_scalars_upload(uint64_t srs_handle, size_t offset, const uint64_t* scalars, size_t scalar_stride,
                              size_t n, int count, uint64_t* scalars_handle_out);
int capgpu_msm_scalars_scatter_dev(uint64_t srs_handle, size_t offset, const void* d_scalars, size_t scalar_stride,
                                   size_t n, int count, uint64_t* scalars_handle_out);
int capgpu_msm_scalars_free(uint64_t scalars_handle);
/* d_out_xyz: count * 96 bytes on the calling thread's device, as capgpu_msm_g1_dev */
int capgpu_msm_g1_resident(uint64_t srs_handle, uint64_t scalars_handle, int scalars_montgomery, void* d_out_xyz);
/* Bytes moved between device contexts (or from the host) by sharded MSMs since capgpu_init - scalar slices and
 * 96-byte partials -, the number of sharded MSM calls, and how many times an SRS or proving key was replicated onto
 * another context.  Any out pointer may be NULL. */
int capgpu_msm_shard_stats(uint64_t* scalar_bytes_out, uint64_t* partial_bytes_out, uint64_t* calls_out,
                           uint64_t* replications_out);

/* Diagnostic: which window table, sort and split `count` MSMs of n points on this SRS would take, as text
 * ("c=15 windows=18 sort=two-level parts=256 n_sub=65536 slice=1").  Tests pin the plan of the BASELINE sizes with
 * it, so that a size limit can never silently move a configuration to a slower path. */
int capgpu_msm_plan(uint64_t srs_handle, size_t n, int count, char* buf, size_t cap);
/* Diagnostic: what one launch runs AFTER its plan is chosen - `sub_msms` (count * parts of capgpu_msm_plan) sub-MSMs of
 * n_sub points on the table of c window bits: item kernels, scan form, digits kernel, msm_accumulate's grid and mode,
 * item length, combine and reduction kernels with their lengths, and the points the reduction writes next to the points
 * reserved for it ("... combine=quad combine_lanes=4 reduce=grid-quad grid_sums=128 slices=16 finish=quad-64
 * partial_points=131 partial_reserved=131").  It is the function the launch itself consults, so the CAPGPU_MSM_* /
 * CAPGPU_ACC_* switches of the process are in it.  Needs no device and no handle; cap of 1024 bytes is enough.
 * CAPGPU_ERR_INVALID_ARG for a null buffer, zero sizes, or window bits the batched plans cannot run (outside 9..16). */
int capgpu_msm_tail_plan(int c, size_t n_sub, int sub_msms, int has_parts, char* buf, size_t cap);

/* out = sum of n Jacobian points (96 B each, host memory): the combine step after the all-gather of a
 * point-range-sharded MSM (replaces the G-1 `GroupProjective::add_assign` a multi-GPU caller would do). */
int capgpu_g1_sum(const uint64_t* points_xyz, size_t n, uint64_t out_xyz[12]);

/* ---- multi-GPU: one process per GPU, MSM sharded by point range -------------------------------
 * The reference parallelises inside one process (rayon, src/utils/params_builder.rs:194-226); a multi-GPU
 * deployment starts one worker process per GPU.  Rank g uploads (or generates) the bases of ITS point range as its
 * SRS and passes the matching scalar slice; every rank runs the whole Pippenger locally down to one point, then ONE
 * exchange step - an RCCL all-gather of the 96-byte partial per MSM on the library stream, device to device over xGMI -
 * and G - 1 group additions on the device give every rank the full result.  (RCCL has no elliptic-curve reduction
 * operator, hence no all-reduce; bucket arrays are never exchanged.)
 *
 * capgpu_comm_unique_id: called by ONE rank; the 128 bytes (an ncclUniqueId) travel to the other ranks by whatever
 * channel the job has (MPI, a socket, torch.distributed - bench.py broadcasts them).  capgpu_comm_init is collective:
 * it returns once all `world` ranks have called it - or fails with CAPGPU_ERR_COMM when they have not arrived within
 * CAPGPU_COMM_TIMEOUT_MS (default 60000).  RCCL is loaded at that moment (dlopen of librccl.so.1; a copy
 * already in the process is reused), so single-GPU users need no RCCL at all.
 * Failures are agreed on: a rank whose local MSM fails still enters the exchange (its status travels with the
 * partials) and every rank returns an error; a rank that never enters it is caught by the same deadline, the
 * communicator is aborted and the call returns CAPGPU_ERR_COMM instead of hanging. */
int capgpu_comm_unique_id(uint8_t id_out[128]);
int capgpu_comm_init(int rank, int world, const uint8_t id[128]);
int capgpu_comm_destroy(void);
/* rank / world of the communicator; world == 0 when there is none */
int capgpu_comm_info(int* rank_out, int* world_out);
/* Test communicator: a world of `world` ranks that THIS process plays one after the other on its device, through the
 * same payload layout, gather buffer and summation kernel as the RCCL path (the all-gather itself becomes a copy into
 * the rank's slot).  capgpu_msm_g1_sharded_dev is then called once per rank (capgpu_comm_loopback_set_rank before each;
 * the call of the last rank leaves the sum), and with capgpu_plonk_shard_msm(1) the prover plays all ranks of every
 * commitment MSM itself.  Lets a 1-GPU box execute the N > 1 code paths. */
int capgpu_comm_init_loopback(int world);
int capgpu_comm_loopback_set_rank(int rank);
/* out (on every rank) = sum over ranks of sum_i scalars_r[i] * bases_r[offset + i]: `count` MSMs in one launch, their
 * partials exchanged in ONE all-gather of count * 96 bytes per rank.  Arguments as capgpu_msm_g1_dev (n_local = this
 * rank's points; may differ between ranks, count may not). */
int capgpu_msm_g1_sharded_dev(uint64_t srs_handle, size_t offset, const void* d_scalars, size_t scalar_stride,
                              size_t n_local, int count, int scalars_montgomery, void* d_out_xyz);
int capgpu_msm_g1_sharded(uint64_t srs_handle, size_t offset, const uint64_t* scalars, size_t n_local,
                          uint64_t out_xyz[12]);
/* BASELINE config 4, mode A: with on != 0 every commitment MSM of capgpu_plonk_preprocess / capgpu_plonk_prove* is cut
 * by point range over the ranks of the communicator (each rank holds the whole commit key, uses its range) and all
 * ranks must then make the same calls with the same inputs; they all return the same proofs.  Mode B - the default,
 * and the faster one for throughput - is replicas: independent proofs on independent ranks, no communicator needed. */
int capgpu_plonk_shard_msm(int on);

/* ---- NTT: replaces Radix2EvaluationDomain::{fft, ifft, coset_fft, coset_ifft}_in_place -------- */
/* in place, natural order in/out, Montgomery Fr; dir: 0 forward, 1 inverse (includes n^-1);
 * coset: 0/1 (generator 5: scale by 5^i before the forward transform / by 5^-i after the inverse).
 * Inputs may be any 256-bit image of their residue (x + r gives the output of x; tests/test_gpu_ntt_plans.py); outputs
 * are canonical (< r). */
int capgpu_ntt_fr(uint64_t* data, uint32_t log_n, int dir, int coset);
int capgpu_ntt_fr_batch(uint64_t* const* data, int count, uint32_t log_n, int dir, int coset);
int capgpu_ntt_fr_dev(void* d_data, size_t stride_elems, int count, uint32_t log_n, int dir, int coset);
/* Diagnostic, as capgpu_msm_plan: how `count` transforms of 2^log_n elements in one call (capgpu_ntt_fr_dev; a batch
 * call is one such call) are launched.  Passes are listed in the order they run, the row pass last; entries beyond
 * `passes` are 0.  A tile is 2^(digits[i] + log_c[i]) <= 2^tile_log elements of LDS.  Reads CAPGPU_NTT_TILE_LOG,
 * CAPGPU_NTT_TILE_ADAPT and CAPGPU_NTT_PERSISTENT as the transforms do (once per process).  Needs no device.  Tests
 * use it to assert which path a shape took. */
typedef struct capgpu_ntt_plan_info {
  uint32_t passes;        /* 0 (log_n = 0: nothing runs), 1, 2 or 3 */
  uint32_t tile_log;      /* log2 of the LDS tile chosen for count << log_n elements */
  uint32_t digits[3];     /* log2 of the sub-transform size of each pass */
  uint32_t log_c[3];      /* log2 of the tile width of each pass */
  uint64_t tiles[3];      /* tiles per array of each pass */
  uint32_t persistent[3]; /* 1: workgroups take tile after tile from a counter (CAPGPU_NTT_PERSISTENT) */
  uint32_t reserved;
} capgpu_ntt_plan_info;
int capgpu_ntt_plan(uint32_t log_n, int count, capgpu_ntt_plan_info* out);

/* ---- PLONK (TurboPlonk, 5 wires, 13 selectors) ------------------------------------------------ */
typedef struct capgpu_proof {
  uint64_t wires_poly_comms[CAPGPU_NUM_WIRE_TYPES][8];      /* affine, Montgomery */
  uint64_t prod_perm_poly_comm[8];
  uint64_t split_quot_poly_comms[CAPGPU_NUM_WIRE_TYPES][8];
  uint64_t opening_proof[8];
  uint64_t shifted_opening_proof[8];
  uint64_t wires_evals[CAPGPU_NUM_WIRE_TYPES][4];           /* Fr, Montgomery */
  uint64_t wire_sigma_evals[CAPGPU_NUM_WIRE_TYPES - 1][4];
  uint64_t perm_next_eval[4];
} capgpu_proof;

typedef struct capgpu_verifying_key {
  uint64_t domain_size;
  uint64_t num_inputs;
  uint64_t k[CAPGPU_NUM_WIRE_TYPES][4];                     /* coset representatives, Montgomery */
  uint64_t selector_comms[CAPGPU_NUM_SELECTORS][8];         /* q_lc x4, q_mul x2, q_hash x4, q_o, q_c, q_ecc */
  uint64_t sigma_comms[CAPGPU_NUM_WIRE_TYPES][8];
} capgpu_verifying_key;

/* selectors: 13 columns of n Fr (Montgomery), column-major, gate order above; sigma_evals: 5 columns
 * of n Fr = sigma_i(omega^j) (the extended permutation as field elements k_i' * omega^j').
 * n must be a power of two, 16 <= n (the quotient is interpolated on 6n points, which must hold its 5n + 8
 * coefficients and the 5 (n + 2) the split-quotient commitments read), n + 3 <= SRS size. */
int capgpu_plonk_preprocess(uint64_t srs_handle, size_t n, size_t num_inputs, const uint64_t* selectors,
                            const uint64_t* sigma_evals, uint64_t* pk_handle_out, capgpu_verifying_key* vk_out);
/* The same with the columns in `input_form` (above): CAPGPU_INPUT_COEFFS takes the 13 selector polynomials and the 5
 * extended-permutation polynomials, n coefficients each (a DensePolynomial shorter than n is zero-padded by the
 * caller), in the same column order. */
int capgpu_plonk_preprocess_ex(uint64_t srs_handle, size_t n, size_t num_inputs, const uint64_t* selectors,
                               const uint64_t* sigmas, int input_form, uint64_t* pk_handle_out,
                               capgpu_verifying_key* vk_out);
/* Key generation from the circuit's wire -> variable table instead of sigma's 5 n field elements: wire_vars is 5 columns
 * of n ids, column-major like the wire columns (the first five of jf-relation's `wire_variables`), every id below num_vars
 * (1 <= num_vars < 2^32; CAPGPU_ERR_INVALID_ARG naming the first offending (wire, row) otherwise; ids that occur in no cell
 * are allowed, num_vars may exceed 5 n).  The extended permutation is built ON THE DEVICE by jf-relation's
 * compute_wire_permutation rule - the cells c = wire * n + row of one variable form a cycle in ascending c, the last cell
 * pointing to the first - from a sort of the unique keys (variable, cell): the result is a function of the table alone.
 * selectors come in selector_form (CAPGPU_INPUT_EVALS / _COEFFS), as in capgpu_plonk_preprocess_ex.  The key, its vk and
 * its capgpu_plonk_key_serialize bytes equal those of capgpu_plonk_preprocess fed the same permutation as sigma_evals.
 * The key keeps the table (4 B x 5 n, device-resident, replicated to a context like the rest of the key) and the index form
 * of the permutation, which the witness check would otherwise derive by one discrete logarithm per cell: it accepts
 * CAPGPU_INPUT_VARS in every entry point that takes an input_form. */
int capgpu_plonk_preprocess_vars(uint64_t srs_handle, size_t n, size_t num_inputs, const uint64_t* selectors,
                                 int selector_form, const uint32_t* wire_vars, size_t num_vars, uint64_t* pk_handle_out,
                                 capgpu_verifying_key* vk_out);
/* Attaches a table to a key made another way - capgpu_plonk_preprocess[_ex], or capgpu_plonk_key_deserialize, whose blob
 * has no place for it - after checking on the device that the permutation the table implies is the key's own, cell for
 * cell: a mismatch is CAPGPU_ERR_INVALID_ARG naming the first differing cell and the key stays as it was.  A key that has
 * a table already takes another one under the same check (ids may be renumbered, not regrouped).  Not to be called while
 * other calls use the key. */
int capgpu_plonk_key_set_vars(uint64_t pk_handle, const uint32_t* wire_vars, size_t num_vars);
/* num_vars of the key's table: the length of a CAPGPU_INPUT_VARS witness; 0 when the key has no table */
int capgpu_plonk_key_num_vars(uint64_t pk_handle, size_t* num_vars_out);

/* ---- Completing a witness on the device (the witness solver) -----------------------------------------------------------
 * A circuit's caller supplies a few thousand values - inputs, constants, hinted bits - and every other variable follows
 * from a gate row.  A key with a wire -> variable table takes the list of GIVEN variable ids and derives, once, the
 * schedule by which the rest is computed; capgpu_plonk_solve_vars* then completes whole batches of assignments on the
 * device.  The result is exactly a CAPGPU_INPUT_VARS witness (canonical Montgomery words, num_vars per witness): it goes
 * unchanged, and in place, into every entry point that takes that form, capgpu_plonk_check_witness* included.
 *
 * THE RULE.  V is the set of valued variables, at first the given ids.  The rows j = 0 .. n-1 are walked in ascending
 * order; U = the distinct variables in the row's five cells that are not in V.  Selectors are the key's selector VALUES
 * on the domain (the table the witness check derives); tests against zero are mod r.
 *   |U| = 0                   the row is a constraint: it defines nothing and is not evaluated (checking stays with
 *                             capgpu_plonk_check_witness*).
 *   j < num_inputs, |U| > 0   refused: a public-input variable must be given.
 *   |U| >= 2                  refused.
 *   U = {u}:
 *     OUT    u sits in wire 4 only, and q_o != 0 or q_ecc != 0:   w4 = rest / (q_o - q_ecc w0 w1 w2 w3),
 *            rest = q_c + sum_i q_lc_i w_i + q_mul0 w0 w1 + q_mul1 w2 w3 + sum_i q_hash_i w_i^5   (i = 0 .. 3).
 *            A row with q_ecc = 0 multiplies by 1 / q_o, computed once at set-up; a row with q_ecc != 0 inverts per
 *            witness.
 *     ROOT5  u sits in exactly one wire i < 4, with q_hash_i != 0, q_lc_i = 0, the q_mul selector of i's pair = 0 and
 *            q_ecc = 0:   w_i = ((q_o w4 - rest without the q_hash_i term) / q_hash_i)^e,  e = 5^-1 mod (r - 1)
 *            (it exists because (r - 1) mod 5 = 1; the library derives e and checks this).  This is Rescue's inverse
 *            S-box gate as jf-relation lays it: the hinted root on an input wire, the known value on wire 4.
 *     any other shape        refused.
 *     Then u joins V.
 * level(given) = 0; level(u) = 1 + the largest level among the other variables of u's row (for ROOT5 that includes wire
 * 4's variable); the rows of one level are independent of each other.  Variables that occur in no cell and are not given
 * come out as 0.
 * Refusals are CAPGPU_ERR_INVALID_ARG at set-up, each naming the lowest offending row and the variable(s); so are a
 * duplicate id in the list, an id at or beyond num_vars, and a key without a table.  The key then stays as it was.
 * Per witness, an OUT row whose denominator is 0 mod r sets its variable to 0 and the witness's status becomes
 * {kind 1, row = the LOWEST such row}; the other witnesses of the call are unaffected.
 *
 * HINTS (capgpu_plonk_key_set_given_hints).  What a circuit builder computes beside its rows - the bits of a value, an
 * inverse, a zero flag - need not be given: a hint gives `count` target variables their values from ONE source variable.
 *   BITS    1 <= count <= 254: c is the canonical integer of src, 0 <= c < r; target i is the field element 0 or 1 equal
 *           to bit i of c.  Bits beyond `count` are dropped silently: the circuit's recomposition row then fails in
 *           capgpu_plonk_check_witness*, which is where checking lives.
 *   INV0    count = 1: src^(r - 2), the chain an OUT row with q_ecc uses; 0 comes out as 0, without a test.
 *   ISZERO  count = 1: 1 if src = 0 mod r, else 0.
 * Firing.  A hint is READY when its src is in V and it has not fired.  Firing takes the ready hint of lowest index; its
 * targets join V with level = 1 + level(src); this repeats until no hint is ready.  Firing runs once before row 0 and
 * again after every row that defines a variable.  A hint whose source is another hint's target chains by this alone.
 * The row walk is unchanged: a row whose variables are all valued is a constraint, so a hinted variable may sit on any
 * wire - jf-relation's unpack / is_zero / is_equal lay theirs on input wires.
 * Items.  A level's kernel items are its defining rows plus its hint items: INV0 and ISZERO one each, a BITS hint
 * ceil(count / 32), item g holding bits 32 g .. 32 g + 31.  Inside a level the items are ordered by (kind, row or hint
 * index, chunk): the rows' three kinds, then INV0 - next to the other exponentiations - then ISZERO, then BITS.
 * capgpu_solver_info: num_defined, inv_rows and root_rows count rows only; levels, widest_level and the median behind the
 * automatic pack width count items.  For a key without hints the schedule is byte for byte the one without this rule.
 * Hint refusals are CAPGPU_ERR_INVALID_ARG at set-up, each naming the hint's index and the variable, the key unchanged:
 * an unknown kind; src or a target at or beyond num_vars; a count out of range for the kind; first + count > num_targets;
 * a target listed twice (in one hint or two); a target equal to its src; a target that is given; a target that already
 * has a value when its hint fires (the defining row is named); a hint whose source never gets a value.  Row refusals are
 * unchanged and still name their lowest row.  No hint sets a status word.
 *
 * MORE RULES, OPT-IN (capgpu_plonk_key_set_solver's flags; 0 is the rule above).  Both touch only rows the rule above
 * refuses: a circuit and list it accepts get the same schedule, byte for byte, under every flag value, and its launches
 * run the kernels they ran.
 *   CAPGPU_SOLVER_LINEAR.  One more shape for U = {u}, tried after OUT and ROOT5:
 *     LIN    u sits in exactly one wire i < 4, with q_lc_i != 0, q_hash_i = 0, the q_mul selector of i's pair = 0 and
 *            q_ecc = 0:   w_i = (q_o w4 - rest without the q_lc_i w_i term) * (1 / q_lc_i),  the constant computed once
 *            at set-up like 1 / q_hash_i.  Disjoint from ROOT5, which wants q_lc_i = 0.  This is enforce_equal(computed,
 *            public) read from right to left, and any linear row with one unknown input.
 *     level(u) = 1 + the largest level among the row's other variables, wire 4 included; hints fire behind a LIN row as
 *     behind any defining row.  Inside a level LIN rows come behind the OUT rows without q_ecc and before every kind that
 *     pays a chain.  capgpu_solver_info.num_defined counts LIN rows; inv_rows and root_rows do not.  A schedule with a LIN
 *     row runs kernels of its own (the hint-capable walk with the LIN case); every other schedule runs what it ran.
 *   CAPGPU_SOLVER_DERIVE_PUBLIC.  A row j < num_inputs is a constraint during the walk whatever it holds: it defines
 *     nothing and is not refused there.  A public-input variable that is not given gets its value from a later row or a
 *     hint - in practice LIN on its enforce_equal row.  After the walk, and after the hints' own check, the LOWEST row
 *     j < num_inputs that still holds a variable without a value is refused, naming the row and the variable.  A public
 *     input that is given is level 0 as before.
 *   The flags are independent; each alone is valid.  Every shape refused without them other than these stays refused with
 *   the same text.  capgpu_solver_rules_info: lin_rows, and derived_inputs = the rows below num_inputs the walk met holding
 *   a variable without a value.
 *
 * TIMING.  Given values are secret.  Both exponentiations of this path - a^(r-2) for the inversion, a^e for the fifth
 * root - walk the bits of a public exponent: 254 squarings and one product per set bit, whatever the base; no
 * variable-time inversion is used per witness.  The constants 1 / q_o and 1 / q_hash_i are functions of the circuit
 * alone.  Which rows run which chain is a property of the circuit, not of the witness.  The one data-dependent step is
 * the zero test of an inverted denominator, whose outcome the status reports anyway.  In a hint item no branch, loop
 * bound or address depends on a witness value: INV0 is the same public-exponent chain without any zero test; BITS takes
 * the canonical integer through the field's fixed-sequence conversion, selects its 32-bit word by a chain of selects
 * over a public chunk number, and stores count-many images (a bound of the circuit), each the words of 1's image times
 * the bit; ISZERO ors the eight words and turns "non-zero" into a bit by a carry, then selects the same way.  A LIN row
 * has no inversion per witness and no zero test: which cell is cleared and that no chain runs follow from the schedule,
 * and 1 / q_lc_i is a function of the circuit alone.  (The paragraph at capgpu_plonk_set_wire_commit describes the prover
 * itself.) */
typedef struct capgpu_solver_info {
  uint64_t num_given;    /* ids in the given list */
  uint64_t num_defined;  /* variables defined by a row */
  uint64_t levels;       /* dependency depth */
  uint64_t widest_level; /* items (rows, and hint items if the key has hints) of the widest level */
  uint64_t inv_rows;     /* OUT rows with q_ecc != 0: one inversion per witness each */
  uint64_t root_rows;    /* ROOT5 rows */
} capgpu_solver_info; /* 48 bytes */
typedef struct capgpu_solve_status {
  uint32_t kind; /* 0 solved, 1 zero denominator at `row` */
  uint32_t reserved;
  uint64_t row;
} capgpu_solve_status; /* 16 bytes */
/* Gives the key its list of given variables and derives the schedule (host pass over the table and the selector values,
 * read back once; one 32-byte constant per defining row).  The schedule lives with the key: replicated to a context on
 * first use like the key's table, replaced by a second call, dropped when capgpu_plonk_key_set_vars changes the table,
 * freed by capgpu_plonk_free_key.  info_out may be NULL.  Not to be called while other calls use the key. */
int capgpu_plonk_key_set_given(uint64_t pk_handle, const uint32_t* given_vars, size_t num_given,
                               capgpu_solver_info* info_out);
/* the schedule's figures; all zero: the key has no solver */
int capgpu_plonk_key_solver_info(uint64_t pk_handle, capgpu_solver_info* info_out);
#define CAPGPU_HINT_BITS 0   /* count targets, 1 <= count <= 254: target i = bit i of the canonical value of src */
#define CAPGPU_HINT_INV0 1   /* count == 1: src^-1 mod r, and 0 for src = 0 */
#define CAPGPU_HINT_ISZERO 2 /* count == 1: 1 if src = 0 mod r, else 0 */
typedef struct capgpu_hint {
  uint32_t kind;  /* CAPGPU_HINT_* */
  uint32_t src;   /* the source variable */
  uint32_t first; /* the hint's targets are targets[first .. first + count) */
  uint32_t count;
} capgpu_hint; /* 16 bytes */
typedef struct capgpu_hint_info {
  uint64_t num_hints;    /* hints in the list */
  uint64_t num_hinted;   /* variables that are a hint's target */
  uint64_t bits_hints;   /* hints of each kind */
  uint64_t inv_hints;
  uint64_t iszero_hints;
  uint64_t hint_items;   /* kernel items the hints add to the levels */
} capgpu_hint_info; /* 48 bytes */
/* capgpu_plonk_key_set_given with a hint list (HINTS above); capgpu_plonk_key_set_given is this call with num_hints == 0.
 * The hint tables are key-resident like the rows: replicated to a context on first use, replaced by a second set-up call
 * (either one), dropped by capgpu_plonk_key_set_vars, freed by capgpu_plonk_free_key.  Every later entry point -
 * capgpu_plonk_solve_vars[_dev], capgpu_plonk_prove_given[_dev|_async], capgpu_plonk_reserve_given,
 * capgpu_plonk_set_solve_pack - uses whatever schedule the key holds; per-call scratch is what it was.  hints may be NULL
 * when num_hints == 0, targets when num_targets == 0; info_out and hint_info_out may be NULL. */
int capgpu_plonk_key_set_given_hints(uint64_t pk_handle, const uint32_t* given_vars, size_t num_given,
                                     const capgpu_hint* hints, size_t num_hints, const uint32_t* targets,
                                     size_t num_targets, capgpu_solver_info* info_out, capgpu_hint_info* hint_info_out);
/* the figures of the key's hints; all zero: no hints */
int capgpu_plonk_key_hint_info(uint64_t pk_handle, capgpu_hint_info* info_out);
#define CAPGPU_SOLVER_LINEAR 1u        /* the LIN shape (MORE RULES above) */
#define CAPGPU_SOLVER_DERIVE_PUBLIC 2u /* public-input variables need not be given */
typedef struct capgpu_solver_rules_info {
  uint64_t flags;          /* the flags the schedule was derived under */
  uint64_t lin_rows;       /* LIN rows */
  uint64_t derived_inputs; /* rows below num_inputs whose variable had no value when the walk met them */
  uint64_t reserved;
} capgpu_solver_rules_info; /* 32 bytes */
/* capgpu_plonk_key_set_given_hints under `flags` (CAPGPU_SOLVER_*); flags == 0 IS that call: the same schedule bytes, the
 * same refusal texts.  A flag bit the library does not know is CAPGPU_ERR_INVALID_ARG, the key unchanged.  The two older
 * set-up calls keep flags == 0. */
int capgpu_plonk_key_set_solver(uint64_t pk_handle, const uint32_t* given_vars, size_t num_given, const capgpu_hint* hints,
                                size_t num_hints, const uint32_t* targets, size_t num_targets, uint32_t flags,
                                capgpu_solver_info* info_out, capgpu_hint_info* hint_info_out);
/* the figures of the flags; all zero: the key has no solver (or one set with flags == 0 on a circuit that needs none) */
int capgpu_plonk_key_solver_rules_info(uint64_t pk_handle, capgpu_solver_rules_info* info_out);
/* THE FORM OF THE SCHEDULE, OPT-IN PER KEY.  Every set-up call above leaves the key in the DIRECT form: the schedule
 * described so far, in which every OUT row with q_ecc != 0 inverts its own denominator - in a chain of Edwards additions
 * one inversion behind the other.  The DEFERRED form carries the variable of such a row as a pair (numerator, denominator)
 * and inverts a whole chain's denominators together when something needs a plain value.  It gives the same words in
 * vars_out and the same status for every witness.  The rule, over the direct schedule's levels in ascending order with a
 * set PENDING of deferred variables, empty at first:
 *   - a row is FRAC-capable if it is an OUT row and every cell i < 4 that holds a pending variable has q_hash_i = 0.  An
 *     OUT row with q_ecc != 0 that is FRAC-capable defines a deferred variable, whatever its inputs are; so does an OUT row
 *     without q_ecc that has a pending input.  The variable joins PENDING behind its level.  Any other OUT row without
 *     q_ecc stays the direct item.
 *   - ROOT5 and LIN rows, an OUT row with a pending variable on a cell with q_hash_i != 0, and every hint item whose
 *     source is pending need plain values: if a level holds such an item, a FLUSH LEVEL goes in front of it that resolves
 *     ALL of PENDING, which is then empty.  Behind the last level a final flush resolves what is left.
 *   - with cell i holding (N_i, D_i), D_i = 1 for a plain variable, D = D0 D1 D2 D3, E_i = the product of the other three,
 *     P = N0 N1 N2 N3 and
 *       R' = q_c D + sum q_lc_i N_i E_i + q_mul0 N0 N1 D2 D3 + q_mul1 N2 N3 D0 D1 + sum over plain i of q_hash_i N_i^5 D
 *     an OUT row without q_ecc gives (R' / q_o, D) and one with q_ecc (R', q_o D - q_ecc P).  If that denominator is
 *     0 mod r the row enters its number into the status word as in the direct form and its pair becomes (0, 1).
 *   - a flush item resolves up to 32 pairs, v = N / D, with ONE inversion (prefix products, one inverse, walk back), in
 *     the process's inverse form (capgpu_fr_set_inverse_form).
 * The denominators live in a side buffer of the context's scratch, 64 bytes per witness and deferred slot (the largest
 * PENDING of the schedule); capgpu_scratch_stats counts it and capgpu_plonk_reserve_given sizes it.  TIMING above holds for
 * this form: which cells are pending and how many pairs an item resolves are properties of the circuit, a cell's
 * denominator is selected by the schedule's mask, and the one data-dependent step is still the zero test of a row's own
 * denominator.
 * capgpu_solver_info, capgpu_hint_info and capgpu_solver_rules_info keep reporting the direct schedule. */
#define CAPGPU_SOLVE_FORM_DIRECT 0
#define CAPGPU_SOLVE_FORM_DEFERRED 1
typedef struct capgpu_solve_form_info {
  uint64_t form;                /* CAPGPU_SOLVE_FORM_* */
  uint64_t deferred_vars;       /* variables carried as a pair (0 in the direct form, like the next three) */
  uint64_t frac_rows;           /* rows evaluated on pairs */
  uint64_t flush_levels;
  uint64_t flush_items;
  uint64_t levels;              /* levels of the schedule the key runs, flush levels included */
  uint64_t inv_levels_direct;   /* levels of the direct schedule that hold an OUT row with q_ecc or an INV0 item */
  uint64_t inv_levels_deferred; /* flush levels + levels that hold an INV0 item */
} capgpu_solve_form_info; /* 64 bytes */
/* Re-derives the key's schedule in `form` from the solver the key holds (a host pass; no device work).  A key without a
 * solver and an unknown form are CAPGPU_ERR_INVALID_ARG, the key unchanged.  capgpu_plonk_key_set_given, _set_given_hints,
 * _set_solver and capgpu_plonk_key_set_vars leave the key in the DIRECT form.  Everything behind the set-up -
 * capgpu_plonk_solve_vars[_dev], capgpu_plonk_prove_given[_dev|_async], capgpu_plonk_prove_given_io*,
 * capgpu_plonk_reserve_given, capgpu_plonk_set_solve_pack, capgpu_plonk_solve_stats - uses the form the key holds.
 * info_out may be NULL.  Not to be called while other calls use the key. */
int capgpu_plonk_key_set_solve_form(uint64_t pk_handle, int form, capgpu_solve_form_info* info_out);
/* the figures of the form the key holds (the last three for either form); all zero: the key has no solver */
int capgpu_plonk_key_solve_form_info(uint64_t pk_handle, capgpu_solve_form_info* info_out);
/* The public inputs of `count` completed assignments (CAPGPU_INPUT_VARS witnesses, count x num_vars): pub[p][j] for
 * j < num_inputs is the value that makes row j hold - the negative of the gate at PI = 0,
 *   q_o w4 - q_ecc w0 w1 w2 w3 w4 - rest      (rest as under OUT above)
 * evaluated from the key's wire -> variable table and selector values, for a general row, not only an IO gate with
 * q_o = 1.  Results are canonical Montgomery words in rows of num_inputs.  The key needs a table, not a solver: any
 * CAPGPU_INPUT_VARS caller can use it.  One kernel, one lane per (witness, row).
 * Replaces: the host pass that computes a note's public inputs (fee, nullifiers, commitments, memo) beside the circuit.
 * capgpu_plonk_pub_inputs: host arrays, staged through the context's scratch; returns when pub_out is written.
 * capgpu_plonk_pub_inputs_dev: device arrays on the calling thread's context; the launch is enqueued on the context's stream
 * (capgpu_set_stream is honoured) and the call returns without waiting, like capgpu_fr_inverse_batch_dev.
 * count == 0 returns CAPGPU_OK and launches nothing (so does a key with num_inputs == 0); a key without a table and a
 * NULL array with count > 0 are CAPGPU_ERR_INVALID_ARG. */
int capgpu_plonk_pub_inputs(uint64_t pk_handle, int count, const uint64_t* vars, uint64_t* pub_out);
int capgpu_plonk_pub_inputs_dev(uint64_t pk_handle, int count, const void* d_vars, void* d_pub_out);
/* Completes `count` assignments.  given: count x num_given field elements (Montgomery), per witness in the order of
 * given_vars, copied to their variables as they are; vars_out: count x num_vars; status_out: count verdicts.  Returns
 * CAPGPU_OK whenever the solve ran - verdicts are in status_out; count == 0 returns CAPGPU_OK and writes nothing.  The
 * solver does not check constraints: a wrong given value yields a completed assignment that capgpu_plonk_check_witness*
 * refuses.  Runs on the calling thread's context and stream (capgpu_set_stream is honoured); scratch comes from the
 * context (capgpu_scratch_stats counts it).  The _dev form reads d_given and writes d_vars_out in device memory. */
int capgpu_plonk_solve_vars(uint64_t pk_handle, int count, const uint64_t* given, uint64_t* vars_out,
                            capgpu_solve_status* status_out);
int capgpu_plonk_solve_vars_dev(uint64_t pk_handle, int count, const void* d_given, void* d_vars_out,
                                capgpu_solve_status* status_out);
/* Witnesses per workgroup of the solver's launches.  One workgroup per witness leaves most of its 256 lanes idle on a
 * circuit whose levels are narrow; a packed launch gives a workgroup W witnesses and lets its lanes stride over a level's
 * (row, witness) items.  The output is word for word the unpacked kernel's, statuses included: a zero denominator in one
 * witness does not touch its neighbours.  w = 1, 2, 4, 8, 16 forces that W; w = 0 (the default; CAPGPU_SOLVE_PACK sets
 * the process default) chooses: the largest power of two <= 16 with W * (median rows per level) <= 256 - fixed when
 * capgpu_plonk_key_set_given derives the schedule - and W <= the largest power of two not above the launch's count.  A
 * launch of one witness always runs unpacked.  Any other w is CAPGPU_ERR_INVALID_ARG.  Process-wide; read when a solve -
 * or a capgpu_plonk_prove_given* call, or its ticket - starts; both calls work before capgpu_init.
 * _stats: counters since capgpu_init - solver launches, the witnesses they completed, launches at W > 1; any pointer may
 * be NULL. */
int capgpu_plonk_set_solve_pack(int w);
int capgpu_plonk_get_solve_pack(int* w_out);
int capgpu_plonk_solve_stats(uint64_t* launches_out, uint64_t* witnesses_out, uint64_t* packed_launches_out);

/* ---- inversion in the scalar field Fr ----------------------------------------------------------------------------------
 * The form of the Fr inversions the solver's launches run (its OUT rows with q_ecc and its INV0 hints) and of the batch
 * calls below.  CAPGPU_INVERSE_FERMAT: x^(r - 2) bit by bit over the public exponent - what every launch ran before this
 * setting existed, and the default.  CAPGPU_INVERSE_GCD: a constant-time extended binary GCD in 26 jumps of 29 divsteps
 * (Bernstein-Yang; the count is the proven bound for 254-bit inputs), the same canonical result for every input, 0 for 0;
 * like the power it has no branch, loop bound or address that depends on a value.  A fifth-root row is a 254-bit power by
 * nature and keeps it in either form.  Replaces: nothing - the setting only selects which kernel instantiation
 * capgpu_plonk_solve_vars[_dev] and capgpu_plonk_prove_given[_dev|_async] launch; the output of either is the same words,
 * statuses included, and no other entry point changes an inversion with it.
 * set: any form but the two is CAPGPU_ERR_INVALID_ARG.  get: form_out NULL is CAPGPU_ERR_INVALID_ARG.  The process default
 * is CAPGPU_INVERSE_FERMAT, or what the environment variable CAPGPU_FR_INVERSE names ("fermat" or "gcd"; any other value
 * counts as fermat).  Process-wide; read when a launch is issued - a switch between two calls on one key needs no new
 * set-up; both calls work before capgpu_init. */
#define CAPGPU_INVERSE_FERMAT 0
#define CAPGPU_INVERSE_GCD 1
int capgpu_fr_set_inverse_form(int form);
int capgpu_fr_get_inverse_form(int* form_out);
/* out[i] = in[i]^-1 mod r for `count` field elements, and 0 for 0.  Elements are the ABI's field images: 8 x 32-bit words
 * (4 x uint64_t), Montgomery form as everywhere; an image that is not canonical is taken mod r; results are canonical.
 * One kernel launch, one element per lane, 256 per workgroup, in the form set above.  in == out is allowed (no other
 * overlap); count == 0 returns CAPGPU_OK and launches nothing; a NULL array with count > 0 is CAPGPU_ERR_INVALID_ARG.
 * Replaces: a host loop over a CPU field library for a column of denominators or a caller's own hints - the ABI had no
 * field inversion of any kind.
 * capgpu_fr_inverse_batch: host arrays; staged through the context's scratch, returns when h_out is written.
 * capgpu_fr_inverse_batch_dev: device arrays on the calling thread's context; the launch is enqueued on the context's
 * stream (capgpu_set_stream is honoured) and the call returns without waiting for it - work enqueued on that stream
 * afterwards sees d_out. */
int capgpu_fr_inverse_batch(const void* h_in, void* h_out, size_t count);
int capgpu_fr_inverse_batch_dev(const void* d_in, void* d_out, size_t count);
/* Launches that hold an Fr inversion - the solver's and the batch calls' - by the form they ran in, since the library was
 * loaded.  What shows that the setting selects a kernel.  Either pointer may be NULL; works before capgpu_init. */
int capgpu_fr_inverse_stats(uint64_t* fermat_launches_out, uint64_t* gcd_launches_out);

int capgpu_plonk_free_key(uint64_t pk_handle);
/* Shape of a resident proving key: the sizes every prove call's arrays must have (wires: count * 5 * domain_size
 * field elements, pub_inputs: count * num_inputs, blinders: count * 13) and the SRS it commits with.  Any out
 * pointer may be NULL. */
int capgpu_plonk_key_info(uint64_t pk_handle, size_t* domain_size_out, size_t* num_inputs_out,
                          uint64_t* srs_handle_out);

/* wires: 5 columns of n Fr (Montgomery), column-major (the finalised circuit's wire assignment);
 * pub_inputs: num_inputs Fr (Montgomery); ext_msg: the caller's transcript init message
 * (src/proof/transfer.rs:178-180) or NULL; blinders: 13 Fr (Montgomery) drawn by the caller's RNG in
 * the order jf-plonk draws them: 2 per wire polynomial (constant, linear), then 3 for the
 * permutation product polynomial. */
int capgpu_plonk_prove(uint64_t pk_handle, const uint64_t* wires, const uint64_t* pub_inputs, size_t num_inputs,
                       const uint8_t* ext_msg, size_t ext_msg_len, const uint64_t* blinders, capgpu_proof* proof_out);
/* Coalescing of concurrent capgpu_plonk_prove calls (off by default).  The reference proves notes from many rayon
 * worker threads, one prove() per note (src/utils/params_builder.rs:194-226); behind one device those calls would run
 * one after the other at single-proof latency.  With window_us > 0, calls for proving keys of one domain size under one
 * SRS (the notes of different kinds the reference proves side by side share batches) that arrive within
 * window_us microseconds of each other (the window restarts with every arrival, 16 windows at most) - or while the
 * device is busy with a previous batch - are gathered (up to max_batch; 0 = 256) and proved as ONE device batch; each caller receives its own proof and its own return code
 * (an unsatisfied witness fails only its owner).  window_us = 0 switches it off. */
int capgpu_plonk_set_coalescing(uint32_t window_us, uint32_t max_batch);
/* How round 1 computes the five wire commitments.  jf-plonk commits to each blinded wire polynomial through its n + 2
 * COEFFICIENTS (KZG10::commit under src/proof/transfer.rs:181-186).  The same group element is
 *     sum_j w_j [L_j(tau)] G + b0 [tau^n - 1] G + b1 [tau^(n+1) - tau] G
 * - an MSM of the column's n VALUES and its two blinders on the Lagrange-form commit key of the domain, which the
 * library derives from the SRS once per (SRS, domain size) by a group inverse transform (cap_amd/csrc/lagrange.hip;
 * 2 x 64 B x (n + 3) x 18-20 window rows of device memory, built by capgpu_plonk_preprocess or by the first proof; the
 * permutation product's commitment is taken the same way, with its three blinders).  The
 * witness values of a CAP circuit are mostly zeros, booleans and range-check limbs (src/circuit/transfer.rs:53-193): as
 * MSM scalars they have at most one non-zero digit where a coefficient has seventeen.  Proof bytes are identical.
 * mode: 1 = from evaluations (the default), 0 = from coefficients, -1 = back to the default (CAPGPU_WIRE_COMMIT=coeffs
 * makes 0 the process default).  Process-wide; takes effect with the next prove call.
 * When the Lagrange-form key cannot be built (device memory) the call commits from coefficients instead of failing.
 *
 * TIMING AND THE SECRET WITNESS - what this library does and does not promise.  Like the arkworks prover it replaces
 * (ark-ec's multi_scalar_mul skips zero scalars and treats ones apart; its field inversions are variable-time) this
 * library is NOT hardened against timing side channels: kernel durations and memory traffic may depend on secret data,
 * and an observer who can time proofs precisely must be kept away by the deployment, not by this code.  What depends on
 * what:
 *  - mode 1 (default): the wire MSMs' scalars are the secret witness values themselves; the bucket sort skips zero digits,
 *    so round 1's duration grows with the number of non-zero 15-bit digits of the witness (zeros, booleans and small
 *    limbs are cheap: the same property the speed-up comes from).  It reveals an aggregate of the witness's sparsity per
 *    proof (per batch, in a batch), not individual values.
 *  - mode 0 (CAPGPU_WIRE_COMMIT=coeffs): the scalars are the blinded polynomials' coefficients - full-width values
 *    whatever the witness holds; round 1's work is then independent of the witness to the degree jf-plonk's own is.  This
 *    is the mode to choose where proof timing is observable by an adversary.
 *  - the permutation product's commitment (either mode) and everything from round 3 on work on challenge-randomised,
 *    full-width data; round 2's one shared inversion runs a fixed-length chain in both modes (it costs nothing).
 * Power, electromagnetic and co-tenant cache channels on a shared GPU are out of scope in both modes. */
int capgpu_plonk_set_wire_commit(int mode);
/* device batches run and proofs made through the coalescer so far */
int capgpu_plonk_coalescing_stats(uint64_t* batches_out, uint64_t* proofs_out);
/* Small batches (count <= CAPGPU_GRAPH_MAX_BATCH, default 16; 0 switches it off) replay their kernel schedule as
 * hipGraphs: the ~100 launches of a proof fall into up to eight segments between the host's transcript steps, or into ONE
 * with the transcript on the device (capgpu_plonk_set_transcript).  The second call with the same key, batch size,
 * buffers and transcript mode captures them; later calls launch the graphs instead.  Proofs are the same bytes either
 * way.  Counters since process start: segments captured (instantiated) and segments replayed. */
int capgpu_plonk_graph_stats(uint64_t* segments_captured_out, uint64_t* segments_replayed_out);
/* Where the Fiat-Shamir transcript of a prove call runs.  Replaces the per-round use of
 * `jf_plonk::transcript::SolidityTranscript` inside `PlonkKzgSnark::prove` (src/proof/transfer.rs:39-45, :181-186).
 *  - CAPGPU_TRANSCRIPT_HOST (the default): after every round the commitments come back to the host, which converts them
 *    to affine, hashes them and sends the challenges - the proving stream is waited for six or seven times per call.
 *  - CAPGPU_TRANSCRIPT_DEVICE: Keccak-256, the challenge arithmetic, Jacobian -> affine of the 13 commitments, zeta's
 *    tables and the linearisation scalars run on the device (cap_amd/csrc/transcript_dev.hpp, one wavefront per proof):
 *    the five rounds are enqueued without a host wait, the proofs come back in this header's layout with ONE copy and
 *    ONE synchronisation, and a small batch replays as one graph segment instead of up to eight.  Proofs are the same bytes.
 *    A witness that does not satisfy its circuit is refused with the same code and message as in host mode, after the
 *    call's single synchronisation instead of after round 3.
 * Every prove entry point honours the mode.  While capgpu_plonk_shard_msm is on, the commitments meet through a
 * host-driven exchange between the ranks and calls use the host transcript whatever the mode says.
 * Process-wide, callable before capgpu_init; takes effect with the next prove call.  CAPGPU_TRANSCRIPT=device|host in
 * the environment sets the initial mode.  An unknown mode returns CAPGPU_ERR_INVALID_ARG. */
#define CAPGPU_TRANSCRIPT_HOST 0
#define CAPGPU_TRANSCRIPT_DEVICE 1
int capgpu_plonk_set_transcript(int mode);
int capgpu_plonk_get_transcript(int* mode_out);
/* Counters since process start: device batches proved (one per context part of a dealt call) and the times those calls
 * made the host wait for the proving stream, from the batch's first launch to its return (the optional witness check
 * of capgpu_plonk_set_precheck, which runs and is waited for before anything is committed to, is not counted).  Either
 * pointer may be NULL. */
int capgpu_plonk_sync_stats(uint64_t* prove_calls_out, uint64_t* stream_waits_out);
/* Keccak-256 (original 0x01 padding, as sha3 0.10.1's Keccak256 under jf-plonk's transcript) of `count` messages by the
 * device transcript's sponge, one wavefront per message: message i is data[offsets[i] .. offsets[i + 1]) (host memory,
 * offsets non-decreasing, each message shorter than 2^31 bytes); digests_out receives count * 32 bytes.  The handle by
 * which the hash kernel is checked on its own. */
int capgpu_keccak256_batch_dev(const uint8_t* data, const uint64_t* offsets, int count, uint8_t* digests_out);
/* Same, `count` independent proofs under one key pipelined on the device; per-proof arrays are
 * consecutive (wires: count * 5 * n, pub_inputs: count * num_inputs, blinders: count * 13).  With several device
 * contexts bound (capgpu_init) and a calling thread that did not bind itself to one, the batch is cut into contiguous
 * parts of at least CAPGPU_DEAL_MIN (default 8) proofs, one per context, proved concurrently; the proofs are those of the
 * undivided call.  On failure the first failing part's code and message are returned and proofs_out is unspecified. */
int capgpu_plonk_prove_batch(uint64_t pk_handle, int count, const uint64_t* wires, const uint64_t* pub_inputs,
                             size_t num_inputs, const uint8_t* ext_msg, size_t ext_msg_len,
                             const uint64_t* blinders, capgpu_proof* proofs_out);
/* Proofs of SEVERAL proving keys in one device batch: pk_handles[i] is the key of proof i.  The reference proves its
 * transfer, mint and freeze notes side by side (TxnsParams::generate_txns, src/utils/params_builder.rs:194-226); on the
 * device, proofs of different circuits over the same evaluation domain share every MSM and NTT launch.  All keys of a
 * call must have the same domain size and come from the same SRS (CAPGPU_ERR_INVALID_ARG otherwise).  wires: count * 5
 * * n field elements; pub_inputs: count rows of num_inputs elements, num_inputs = the largest public-input count among
 * the keys - a key with fewer inputs uses the first of its row, the rest is ignored; ext_msgs / ext_msg_lens: one
 * transcript init message per proof, or NULL; blinders: count * 13.  Every proof is bit-identical to the one
 * capgpu_plonk_prove makes for the same inputs. */
int capgpu_plonk_prove_multi(const uint64_t* pk_handles, int count, const uint64_t* wires, const uint64_t* pub_inputs,
                             size_t num_inputs, const uint8_t* const* ext_msgs, const size_t* ext_msg_lens,
                             const uint64_t* blinders, capgpu_proof* proofs_out);
int capgpu_plonk_prove_multi_dev(const uint64_t* pk_handles, int count, const void* d_wires, const uint64_t* pub_inputs,
                                 size_t num_inputs, const uint8_t* const* ext_msgs, const size_t* ext_msg_lens,
                                 const uint64_t* blinders, capgpu_proof* proofs_out);
/* Device-resident witness form used by the benchmark (inputs already in HBM). */
int capgpu_plonk_prove_batch_dev(uint64_t pk_handle, int count, const void* d_wires, const uint64_t* pub_inputs,
                                 size_t num_inputs, const uint8_t* ext_msg, size_t ext_msg_len,
                                 const uint64_t* blinders, capgpu_proof* proofs_out);

/* The prove entry points with the wire columns in `input_form` (above).  CAPGPU_INPUT_COEFFS: `wires` holds, per proof,
 * the 5 UNBLINDED wire polynomials of n coefficients (jf-relation's compute_wire_polynomials; the blinders are added on
 * the device as before).  Everything else - layouts, batching over contexts, coalescing (calls of different forms are
 * gathered separately), errors - is that of the entry point without _ex, which is the _ex one with CAPGPU_INPUT_EVALS. */
/* CAPGPU_INPUT_VARS: `wires` holds, per proof, num_vars field elements (capgpu_plonk_key_num_vars; Montgomery) - the value
 * of variable v at index v -, proofs consecutive; _multi takes rows of the LARGEST num_vars among the call's keys, a key
 * with fewer variables using the first of its row, as pub_inputs rows work.  Host-resident input is staged as count *
 * num_vars * 32 bytes through the chunks, part order and copy streams the wire columns take, and one gather per chunk
 * (w[i][j] = vars[wire_vars[i][j]]) writes the columns where the evals form would have copied them; the _dev forms read a
 * device buffer of count * num_vars elements and never write it.  A key without a table refuses the form before the
 * device is touched (tickets: at submission): CAPGPU_ERR_INVALID_ARG, "key has no variable table". */
int capgpu_plonk_prove_ex(uint64_t pk_handle, const uint64_t* wires, const uint64_t* pub_inputs, size_t num_inputs,
                          const uint8_t* ext_msg, size_t ext_msg_len, const uint64_t* blinders, int input_form,
                          capgpu_proof* proof_out);
int capgpu_plonk_prove_batch_ex(uint64_t pk_handle, int count, const uint64_t* wires, const uint64_t* pub_inputs,
                                size_t num_inputs, const uint8_t* ext_msg, size_t ext_msg_len,
                                const uint64_t* blinders, int input_form, capgpu_proof* proofs_out);
int capgpu_plonk_prove_multi_ex(const uint64_t* pk_handles, int count, const uint64_t* wires,
                                const uint64_t* pub_inputs, size_t num_inputs, const uint8_t* const* ext_msgs,
                                const size_t* ext_msg_lens, const uint64_t* blinders, int input_form,
                                capgpu_proof* proofs_out);
int capgpu_plonk_prove_multi_dev_ex(const uint64_t* pk_handles, int count, const void* d_wires,
                                    const uint64_t* pub_inputs, size_t num_inputs, const uint8_t* const* ext_msgs,
                                    const size_t* ext_msg_lens, const uint64_t* blinders, int input_form,
                                    capgpu_proof* proofs_out);
int capgpu_plonk_prove_batch_dev_ex(uint64_t pk_handle, int count, const void* d_wires, const uint64_t* pub_inputs,
                                    size_t num_inputs, const uint8_t* ext_msg, size_t ext_msg_len,
                                    const uint64_t* blinders, int input_form, capgpu_proof* proofs_out);

/* ---- asynchronous proving: tickets ---------------------------------------------------------------------------------
 * Every prove entry point above returns when its proofs are made, so a caller with its witnesses in host memory pays the
 * fill and the drain of the device once per call: one thread proving 256 host witnesses per call reaches 0.95 - 0.97 of
 * the resident rate, two threads bound to two contexts (capgpu_set_device), each proving half, 0.995.  A TICKET is such a
 * bound caller inside the library: submission checks the arguments and returns at once; a worker thread of the library
 * takes a context - the submitting thread's bound one, else a free one, else the round-robin pick - and proves the WHOLE
 * batch there (it is not cut over contexts, and coalescing is not involved); capgpu_wait collects the result.  One thread
 * that keeps two tickets in flight - submit A, submit B, wait A, submit C, wait B, ... - is the two-callers pattern without
 * threads of the caller's own.
 *
 * Submission.  Arguments as capgpu_plonk_prove_batch_ex / _multi_ex.  Every check those calls make before they touch the
 * device is made now, with the same code and message (input form, null pointers, unknown key, the public-input count, keys
 * of different domain sizes or SRS in _multi); a failed check creates no ticket.  count == 0: CAPGPU_OK and ticket 0,
 * which capgpu_wait reports as done.  The transcript messages and the pk_handles array are COPIED.  `wires`,
 * `pub_inputs`, `blinders` and `proofs_out` are BORROWED: the caller keeps them alive and neither writes the inputs nor
 * touches proofs_out until capgpu_wait has reported the ticket done.  The ticket shares ownership of its key(s):
 * capgpu_plonk_free_key with a ticket outstanding is safe, and the ticket is still proved.
 * Tickets of a device start in submission order, at most CAPGPU_ASYNC_INFLIGHT (environment, default 2) of them run at
 * once per physical device, later ones queue.  With 64 tickets outstanding - queued, running, or done and not yet waited
 * for - a submission returns CAPGPU_ERR_BUSY instead of blocking.  The process-wide modes (capgpu_plonk_set_transcript,
 * _set_wire_commit, _set_precheck) are read when the ticket STARTS, as a synchronous call made at that moment would read
 * them; changing them with tickets outstanding is unspecified.  While capgpu_plonk_shard_msm is on, submission returns
 * CAPGPU_ERR_INVALID_ARG: the ranks must prove in lock step.  The worker threads (at most CAPGPU_ASYNC_INFLIGHT per
 * device) are created with the first ticket. */
int capgpu_plonk_prove_batch_async(uint64_t pk_handle, int count, const uint64_t* wires, const uint64_t* pub_inputs,
                                   size_t num_inputs, const uint8_t* ext_msg, size_t ext_msg_len,
                                   const uint64_t* blinders, int input_form, capgpu_proof* proofs_out,
                                   uint64_t* ticket_out);
int capgpu_plonk_prove_multi_async(const uint64_t* pk_handles, int count, const uint64_t* wires,
                                   const uint64_t* pub_inputs, size_t num_inputs, const uint8_t* const* ext_msgs,
                                   const size_t* ext_msg_lens, const uint64_t* blinders, int input_form,
                                   capgpu_proof* proofs_out, uint64_t* ticket_out);
/* Waits for a ticket, from any thread, for at most timeout_ms milliseconds (0 polls, UINT32_MAX: no limit) - blocked on
 * a condition variable, never spinning.
 *  - not done in time: CAPGPU_OK with *done_out = 0; the ticket stays valid;
 *  - done: *done_out = 1, the return value is the proving call's own code and capgpu_last_error() of the CALLING thread
 *    its message - an unsatisfied witness gives the code and text the synchronous call gives in the transcript / precheck
 *    mode the ticket ran in.  The ticket is then CONSUMED;
 *  - unknown or consumed ticket: CAPGPU_ERR_BAD_HANDLE.  Of two threads waiting for one ticket one gets the result, the
 *    other CAPGPU_ERR_BAD_HANDLE.
 * Tickets may be waited for in any order.  capgpu_shutdown lets running tickets finish, drops queued ones (a thread blocked
 * in capgpu_wait receives CAPGPU_ERR_NOT_INITIALISED for them), discards results nobody waits for and joins the workers
 * before any context goes.  capgpu_trim sees a context with a running ticket as busy. */
int capgpu_wait(uint64_t ticket, uint32_t timeout_ms, int* done_out);
/* Counters since capgpu_init: tickets accepted, tickets finished (dropped ones included), and the most tickets that were
 * running at the same moment on one device.  Any pointer may be NULL. */
int capgpu_async_stats(uint64_t* submitted_out, uint64_t* completed_out, uint32_t* max_running_out);
/* Sizes context `slot` (-1: every context) AHEAD for a batch of `count` host-resident proofs under this key in
 * `input_form`, without proving anything: every scratch buffer such a batch would grow - the prover's workspace, the MSM
 * workspace, the NTT scratch, the staging of the witnesses, with capgpu_plonk_set_precheck on the check's scratch - and the
 * pinned result area, in the transcript / wire-commit / precheck modes in force NOW, from the same size expressions the
 * prover uses.  The key, its SRS and the Lagrange-form commit key are brought to that context as the first proof would
 * bring them.  No kernel of the prover runs (capgpu_plonk_sync_stats does not move).  A steady-state call - synchronous
 * from a thread bound to that context, or a ticket that runs there - of at most `count` proofs then allocates nothing:
 * capgpu_scratch_stats stays where it was.  (A synchronous call of an UNBOUND thread is cut into parts, each smaller than
 * the call: reserve the contexts for the call's size, or the part's.)  Buffers get the usual 25 % slack; the call respects
 * capgpu_set_memory_limit and fails as a proving call would: CAPGPU_ERR_OOM naming the bytes. */
int capgpu_plonk_reserve(uint64_t pk_handle, int count, int input_form, int slot);

/* ---- witness check: replaces Circuit::check_circuit_satisfiability as the reference's prove() calls it ------------
 * The reference checks every witness against its circuit BEFORE it calls the SNARK (src/proof/transfer.rs:167-177,
 * mint.rs and freeze.rs likewise) and names the constraint that failed.  The prove entry points above do not: they notice
 * an unsatisfied witness only after round 3, as a quotient of the wrong degree, which names no gate and costs a batch
 * more than half its work.  These calls are that check on the device: every gate (spec eq. (1) with the public input of
 * the row) and every copy constraint w[i][j] == w[i'][j'], sigma_i(omega^j) = k_i' omega^j', for `count` witnesses at
 * once.  Verdict per witness: the first failing gate in row order or, when every gate holds, the first violated copy
 * constraint in (wire, row) order - and how many gates and copy constraints fail in all.  The same on every run.
 *
 * Arguments as the prove entry point of the same suffix (wires: count * 5 * n field elements in `input_form`, never
 * written - coefficient-form input is transformed to values in scratch; pub_inputs: count rows of num_inputs; _multi:
 * one key per witness, rows of the largest public-input count); the same mistakes get the same codes.  The calls return
 * CAPGPU_OK whenever the check RAN - the verdicts are in faults_out - and run on the calling context's stream
 * (capgpu_set_stream); host-resident batches are dealt over the contexts as capgpu_plonk_prove_batch deals them.
 * The first check of a key derives two tables from it on the device and keeps them with the key until
 * capgpu_plonk_free_key: the 13 selector columns' VALUES on the domain (13 * 32 B * n: 13.6 MB at n = 2^15) and the index
 * form of the permutation (4 B * 5 n), one discrete logarithm per cell.  A key whose sigma holds a value in none of the
 * five cosets k_i H is refused by every check: CAPGPU_ERR_INVALID_ARG, "sigma is not a permutation of the extended
 * domain". */
typedef struct capgpu_witness_fault {
  uint32_t kind;            /* 0 satisfied, 1 gate, 2 copy constraint */
  uint32_t wire, wire2;     /* copy: cell (wire,row) must equal (wire2,row2); gate: 0 */
  uint32_t reserved;
  uint64_t row, row2;
  uint64_t gates_failed, copies_failed;
} capgpu_witness_fault;     /* 48 bytes */

/* CAPGPU_INPUT_VARS: the values are gathered into columns (scratch) and only the gates are checked - a witness gathered
 * through the key's table satisfies every copy constraint by construction: copies_failed is 0 and kind is never 2; the
 * gate verdict is that of the expanded columns.  A key with a table needs no discrete logarithms for the other forms
 * either: it has the permutation's index form from its table. */
int capgpu_plonk_check_witness(uint64_t pk_handle, const uint64_t* wires, const uint64_t* pub_inputs, size_t num_inputs,
                               int input_form, capgpu_witness_fault* fault_out);
int capgpu_plonk_check_witness_batch(uint64_t pk_handle, int count, const uint64_t* wires, const uint64_t* pub_inputs,
                                     size_t num_inputs, int input_form, capgpu_witness_fault* faults_out);
int capgpu_plonk_check_witness_batch_dev(uint64_t pk_handle, int count, const void* d_wires, const uint64_t* pub_inputs,
                                         size_t num_inputs, int input_form, capgpu_witness_fault* faults_out);
int capgpu_plonk_check_witness_multi(const uint64_t* pk_handles, int count, const uint64_t* wires,
                                     const uint64_t* pub_inputs, size_t num_inputs, int input_form,
                                     capgpu_witness_fault* faults_out);
/* on != 0: every prove entry point (direct, _batch, _multi, _dev, _ex, small batches replayed as graphs, coalesced
 * calls) runs the check on its staged witnesses first - ahead of the Lagrange-form commit key a domain's first proof may
 * have to build, the workspace and every MSM and NTT of the proof (the check's own work: the first check of a key derives
 * the key's two tables, coefficient-form witnesses take one forward transform into scratch).  A batch with faults
 * returns CAPGPU_ERR_PROOF and a message with the number of bad proofs, the first one and its fault in the reference's
 * wording ("... 2 of 8 witnesses do not satisfy their circuit; first: proof 3: gate 1234 not satisfied", "proof 3: copy
 * constraint (2,40) -> (0,7) violated").  A coalesced call with a bad witness fails alone, with its own message; the
 * other calls of its batch are proved as ONE batch (without the check the batch is proved once as well, in outcome mode
 * - see capgpu_plonk_prove_each -, and the bad call fails with the degree check's message).
 * Host-resident witnesses are then copied in one go instead of chunk by chunk under round 1.  Off (the default):
 * nothing changes.  Process-wide; takes effect with the next prove call. */
int capgpu_plonk_set_precheck(int on);
/* Counters since capgpu_init: bytes of witness input (wire columns, wire polynomials or variable values) that prove and
 * check calls copied from host to device, and launches of the variable form's gather kernel.  _dev calls copy no witness.
 * Either pointer may be NULL. */
int capgpu_plonk_input_stats(uint64_t* witness_bytes_h2d_out, uint64_t* gather_launches_out);

/* ---- per-proof outcomes: a batch is proved PAST its unsatisfied witnesses -------------------------------------------
 * The batch entry points above are all-or-nothing: one unsatisfied witness fails the call for every proof.  The
 * reference's callers are a map of one prove() per note, each with a Result of its own (src/utils/params_builder.rs:
 * 194-226, src/proof/transfer.rs:159-188); these calls are that map as ONE batch.  Arguments, layouts, input forms and
 * argument checks are those of capgpu_plonk_prove_multi_ex / _multi_dev_ex / _multi_async (same codes, same messages; the
 * pointer checks are made before a device is looked for), plus outcomes_out: `count` records, NULL with count > 0 is
 * CAPGPU_ERR_INVALID_ARG.  A call whose pk_handles all name one key makes the launches of capgpu_plonk_prove_batch_ex.
 * Host-resident calls are dealt over the contexts as capgpu_plonk_prove_batch deals them; each part fills its slice.
 *
 * Return value: CAPGPU_OK whenever the batch RAN (the convention of capgpu_plonk_check_witness*); argument errors,
 * CAPGPU_ERR_OOM, HIP errors and CAPGPU_ERR_BUSY fail the call as they fail the others.  count == 0: CAPGPU_OK, nothing
 * written.  Per proof: status is CAPGPU_ERR_PROOF exactly when degree_flags != 0 || fault.kind != 0.  A proof with status
 * CAPGPU_OK is bit for bit what capgpu_plonk_prove_ex makes from the same inputs.  The record of a failed proof is
 * all-ones words - no verifier accepts it (its points and scalars are out of range), so a caller that forgets to look at
 * the status cannot ship it.  By default a failing witness rides the batch to the end and is blanked; with the witness
 * check on and EVERY witness refused the call returns after the check, before the prover reserves anything.  With
 * capgpu_plonk_set_compaction on as well, the witnesses the check refused leave the batch before round 1 (see there).
 * Both transcript homes, both wire-commit modes, all three input forms, graphs for small batches and capgpu_set_stream
 * are honoured; while capgpu_plonk_shard_msm is on the three calls return CAPGPU_ERR_INVALID_ARG (the ranks' lock step has
 * no per-proof exit). */
typedef struct capgpu_prove_outcome {
  int32_t status;             /* CAPGPU_OK, or CAPGPU_ERR_PROOF: this witness does not satisfy its circuit */
  uint32_t degree_flags;      /* the degree check's word for this proof (0 = the quotient had its degree) */
  capgpu_witness_fault fault; /* capgpu_plonk_set_precheck on: the check's verdict; off: kind 0 */
} capgpu_prove_outcome;       /* 56 bytes */

int capgpu_plonk_prove_each(const uint64_t* pk_handles, int count, const uint64_t* wires, const uint64_t* pub_inputs,
                            size_t num_inputs, const uint8_t* const* ext_msgs, const size_t* ext_msg_lens,
                            const uint64_t* blinders, int input_form, capgpu_proof* proofs_out,
                            capgpu_prove_outcome* outcomes_out);
int capgpu_plonk_prove_each_dev(const uint64_t* pk_handles, int count, const void* d_wires, const uint64_t* pub_inputs,
                                size_t num_inputs, const uint8_t* const* ext_msgs, const size_t* ext_msg_lens,
                                const uint64_t* blinders, int input_form, capgpu_proof* proofs_out,
                                capgpu_prove_outcome* outcomes_out);
/* The ticket form (see capgpu_plonk_prove_multi_async): outcomes_out is BORROWED like proofs_out until capgpu_wait has
 * reported the ticket done; capgpu_wait returns CAPGPU_OK for a ticket that ran, whatever its outcomes say. */
int capgpu_plonk_prove_each_async(const uint64_t* pk_handles, int count, const uint64_t* wires,
                                  const uint64_t* pub_inputs, size_t num_inputs, const uint8_t* const* ext_msgs,
                                  const size_t* ext_msg_lens, const uint64_t* blinders, int input_form,
                                  capgpu_proof* proofs_out, capgpu_prove_outcome* outcomes_out, uint64_t* ticket_out);
/* ---- a Vec of notes whose keys have SEVERAL domain sizes (or SRS) in one call --------------------------------------------
 * The reference proves a Vec<TransactionNote> of transfers, mints and freezes under one into_par_iter()
 * (src/utils/params_builder.rs:64-241); the mint's domain is half the others'.  One device batch holds keys of one domain
 * size under one SRS, so capgpu_plonk_prove_each refuses that Vec; these calls take it.  The notes are cut into GROUPS -
 * all notes whose keys share (domain size, SRS), numbered by first appearance, members in the caller's order - and every
 * group is proved as ONE batch, exactly as capgpu_plonk_prove_each proves it.
 * These are outcome calls: everything capgpu_plonk_prove_each[_dev,_async] says about the return value (CAPGPU_OK whenever
 * the batch ran), the all-ones record of a failed proof, capgpu_prove_outcome[_text], borrowed ticket pointers, the pointer
 * checks before a device is looked for, capgpu_plonk_shard_msm (CAPGPU_ERR_INVALID_ARG) and count == 0 holds here too.
 *   WITNESSES, host form.  wires[i] points to note i's own witness as capgpu_plonk_prove_ex takes it for that key:
 *   5 n_i elements (CAPGPU_INPUT_EVALS / _COEFFS), or the key's num_vars values (CAPGPU_INPUT_VARS) - not padded to the
 *   call's largest.  The blocks are read where they are: no host copy is made to bring a group together.
 *   WITNESSES, device form.  wire_offsets[i] is the offset of note i's block, in field elements (32 bytes), from d_wires;
 *   blocks have the lengths above and may lie in any order.  d_wires must be 16-byte aligned.  The buffer is never written.
 *   pub_inputs, blinders: capgpu_plonk_verify_block_dev's convention - `count` rows of num_inputs, at least the largest
 *   count among ALL the call's keys, a key with fewer inputs using the first of its row; blinders is count * 13.  The arrays a
 *   notes call took and the proofs it wrote go into the block verifier as they are.
 *   ORDER OF THE CHECKS.  (1) an unknown input_form; (2) the pointers: count < 0, or count > 0 with a NULL pk_handles,
 *   wires (d_wires, wire_offsets), blinders, proofs_out or outcomes_out, a NULL pub_inputs with num_inputs > 0, ext_msgs
 *   without ext_msg_lens, a NULL ticket_out: "capgpu_plonk_prove_notes: bad argument"; (3) host form: a NULL wires[i]
 *   ("capgpu_plonk_prove_notes: wires[i] is NULL"); device form: a d_wires that is not 16-byte aligned - all
 *   CAPGPU_ERR_INVALID_ARG and made before a device is looked for; (4) CAPGPU_ERR_NOT_INITIALISED; (5) count == 0: CAPGPU_OK,
 *   nothing written; (6) capgpu_plonk_shard_msm on; (7) the keys, note by note: an unknown handle (CAPGPU_ERR_BAD_HANDLE), a
 *   key of the reference-schedule test mode (CAPGPU_RECOMPUTE_PK_COSET), CAPGPU_INPUT_VARS with a key that has no table;
 *   (8) num_inputs smaller than the largest count among the keys ("capgpu_plonk_prove_notes: rows of A public inputs
 *   given, the keys need B").  Two faults at once give the earlier one.
 *   THE CONTRACT.  For every note i, proofs_out[i] and outcomes_out[i] are bit for bit what capgpu_plonk_prove_each writes
 *   for that note when called with the notes of i's group alone, in the same modes; a surviving proof is therefore the lone
 *   capgpu_plonk_prove_ex's.  A call whose keys form ONE group goes down capgpu_plonk_prove_each's own path: same launches,
 *   same dealing in contiguous cuts, same graph signatures.
 *   HOW A CALL RUNS.  Groups START by count * n descending (ties: group number).  Host form, unbound thread, more than one
 *   context, two or more groups: every group is one part, whole, on a context of its own - at most as many at a time as
 *   capgpu_plonk_prove_each cuts a batch into, the idle contexts first in slot order; a context that finishes takes the
 *   next group.  A bound thread, a single context, an entry from inside the library: the groups run one after the other on
 *   that context.  A ticket runs whole on the context its worker got; keys and messages are copied at submission.  The
 *   device form runs on the calling thread's context and stream: a group whose members' blocks lie at ONE constant stride
 *   in member order (evals / coeffs: exactly 5 n; variables: any constant stride of at least the group's largest num_vars)
 *   is proved where it lies - capgpu_plonk_prove_each_dev's rules, compaction's among them -; any other group is gathered
 *   into library staging by one copy kernel and is "library staging" from there on.  Precheck, compaction (per group),
 *   both transcript homes, both wire-commit modes, graphs, capgpu_set_stream and capgpu_set_memory_limit are honoured.
 *   ERRORS.  A group that fails with a code (CAPGPU_ERR_OOM, HIP) does not stop the groups already running; the call
 *   returns the code and message of the first failed group in run order, and what proofs_out holds is then unspecified.
 * capgpu_plonk_notes_plan needs no device: it reports the groups such a call would form (records in group order; cap smaller
 * than their number fills cap records and still reports the number) and, group_of_out not NULL, every note's group.
 * capgpu_plonk_reserve_notes sizes context `slot` (-1: every context) for the largest need over the call's groups in the
 * modes in force, host and device form (the gather's staging included), and brings every key, its SRS and its
 * Lagrange-form commit key there: a following notes call of the same shape leaves capgpu_scratch_stats where it was.
 * capgpu_plonk_notes_stats: process-wide counters since capgpu_init; `out` must not be NULL.
 * LEFT OUT: given-value and all-or-nothing forms over several domain sizes; the device form's groups on sibling contexts;
 * splitting one heavy group beside a light one; any mixing of domain sizes inside a launch. */
typedef struct capgpu_notes_group {
  uint64_t srs_handle;
  uint64_t domain_size;
  uint32_t count;      /* notes of the group */
  uint32_t first;      /* its lowest note index */
  uint32_t max_inputs; /* the largest num_inputs among its keys */
  uint32_t run_order;  /* 0: starts first */
} capgpu_notes_group;  /* 32 bytes */
typedef struct capgpu_notes_stats {
  uint64_t calls;               /* notes calls (tickets when they run) that got past their checks */
  uint64_t groups;              /* groups they proved */
  uint64_t groups_dealt;        /* ... of which on a context the deal chose, not the caller's own */
  uint64_t contexts_dealt;      /* contexts those deals used, summed over the calls */
  uint64_t dev_groups_direct;   /* device form: groups proved where they lay, without a copy */
  uint64_t dev_groups_gathered; /* device form: groups gathered into library staging ... */
  uint64_t rows_gathered;       /* ... and the rows that moved */
} capgpu_notes_stats;           /* 56 bytes */
int capgpu_plonk_prove_notes(const uint64_t* pk_handles, int count, const uint64_t* const* wires,
                             const uint64_t* pub_inputs, size_t num_inputs, const uint8_t* const* ext_msgs,
                             const size_t* ext_msg_lens, const uint64_t* blinders, int input_form,
                             capgpu_proof* proofs_out, capgpu_prove_outcome* outcomes_out);
int capgpu_plonk_prove_notes_dev(const uint64_t* pk_handles, int count, const void* d_wires, const uint64_t* wire_offsets,
                                 const uint64_t* pub_inputs, size_t num_inputs, const uint8_t* const* ext_msgs,
                                 const size_t* ext_msg_lens, const uint64_t* blinders, int input_form,
                                 capgpu_proof* proofs_out, capgpu_prove_outcome* outcomes_out);
int capgpu_plonk_prove_notes_async(const uint64_t* pk_handles, int count, const uint64_t* const* wires,
                                   const uint64_t* pub_inputs, size_t num_inputs, const uint8_t* const* ext_msgs,
                                   const size_t* ext_msg_lens, const uint64_t* blinders, int input_form,
                                   capgpu_proof* proofs_out, capgpu_prove_outcome* outcomes_out, uint64_t* ticket_out);
int capgpu_plonk_notes_plan(const uint64_t* pk_handles, int count, capgpu_notes_group* groups_out, size_t cap,
                            size_t* num_groups_out, uint32_t* group_of_out);
int capgpu_plonk_reserve_notes(const uint64_t* pk_handles, int count, int input_form, int slot);
int capgpu_plonk_notes_stats(capgpu_notes_stats* out);
/* ---- proving from the values a circuit is GIVEN -----------------------------------------------------------------------
 * One call from given values to proofs: the solver (capgpu_plonk_key_set_given) and the variable-form outcome call, fused.
 * These are outcome calls: everything capgpu_plonk_prove_each[_dev,_async] says about arguments, layouts, the return value
 * (CAPGPU_OK whenever the batch ran), the all-ones record of a failed proof and borrowed ticket pointers holds here too.
 * What differs:
 *   INPUT.  given holds, per proof, the values of its key's given list in given_vars order (Montgomery), proofs
 *   consecutive.  With several keys the rows have the largest num_given among the call's keys and a key with fewer uses
 *   the first of its row - as pub_inputs and variable-form rows do.  The _dev form reads d_given in device memory and
 *   never writes it.
 *   SOLVER STATUS.  solved_out may be NULL; otherwise it receives `count` records, exactly what capgpu_plonk_solve_vars
 *   reports for that witness.  A zero-denominator witness is not treated specially: its variable is 0 and it goes on as
 *   it is; its outcome is what the witness check or the degree check says about the completed assignment.
 *   REFUSALS, before a device is touched (tickets: at submission): a key without a solver is CAPGPU_ERR_INVALID_ARG
 *   ("capgpu_plonk_prove_given: the key has no solver (capgpu_plonk_key_set_given gives it one)"); NULL given, blinders,
 *   proofs_out or outcomes_out with count > 0; keys of different domain size or SRS, as capgpu_plonk_prove_each refuses
 *   them; capgpu_plonk_shard_msm on.  count == 0 returns CAPGPU_OK and writes nothing.
 *   MECHANISM.  The given values are staged in one copy of count * num_given * 32 bytes (capgpu_plonk_input_stats' byte
 *   counter grows by exactly that; _dev: by nothing).  The solver runs on the proving stream into library scratch, packed
 *   as capgpu_plonk_set_solve_pack says, one launch per distinct key over that key's proofs.  From there the call IS the
 *   variable-form outcome call on a library-owned buffer: gather, optional witness check, optional compaction (the rules
 *   of "variable form in library staging"), five rounds.  The status words come back with the proofs: with the transcript
 *   on the device, capgpu_plonk_sync_stats' stream_waits moves as for capgpu_plonk_prove_each_dev of the solved buffer.
 *   Host-resident calls of an unbound thread are dealt over the contexts as capgpu_plonk_prove_each deals them, each part
 *   solving its slice on its own context.  A ticket runs whole on one context: two tickets in flight are a solve on one
 *   context beside a prove on the other.
 *   THE CONTRACT.  For every proof i, proofs_out[i] and outcomes_out[i] are bit for bit what capgpu_plonk_solve_vars_dev
 *   followed by capgpu_plonk_prove_each_dev(..., CAPGPU_INPUT_VARS, ...) make of the same inputs in the same modes, and
 *   solved_out[i] is that solve's status.
 * capgpu_plonk_reserve_given sizes what capgpu_plonk_reserve(pk_handle, count, CAPGPU_INPUT_VARS, slot) sizes and, from the
 * call's own size expressions, the staging of the given values, the solved buffer and the status words, and brings the
 * key's schedule to the context: a steady-state call of at most `count` proofs then leaves capgpu_scratch_stats where it
 * was.
 * WITHOUT PASSING PUBLIC INPUTS (capgpu_plonk_prove_given_io[_dev|_async]).  capgpu_plonk_prove_given* with two changes:
 * the pub_inputs parameter is gone, and pub_inputs_out (host memory, count rows of num_inputs, before proofs_out) receives
 * what the library proved against.  Any key with a solver is taken; the flags above are not required.  Everything else
 * about arguments, refusals, outcomes, tickets and borrowed pointers (pub_inputs_out among them) is prove_given's.
 *   THE CONTRACT.  pub_inputs_out[i] is what capgpu_plonk_pub_inputs_dev makes of proof i's solved assignment (a key with
 *   fewer public inputs than the row: zeros behind its own); proofs_out[i], outcomes_out[i] and solved_out[i] are bit for bit
 *   what capgpu_plonk_solve_vars_dev, capgpu_plonk_pub_inputs_dev and capgpu_plonk_prove_each_dev(..., CAPGPU_INPUT_VARS, ...)
 *   with those public inputs make of the same inputs in the same modes.  A failed proof's record is all ones as ever; its
 *   pub_inputs_out row is still the computed one.
 *   MECHANISM.  Behind the solver's launches one k_pub_inputs launch per distinct key gathers the rows on the device; they
 *   come to the host with ONE stream wait more than capgpu_plonk_prove_given takes, and the call goes on as that call on
 *   the host buffer.  That wait is made by this call, not by the prover: capgpu_plonk_sync_stats moves exactly as for
 *   capgpu_plonk_prove_given (its stream_waits does not count the extra wait).
 *   capgpu_plonk_reserve_given sizes the staging of these rows too, for a key whose solver was set with
 *   CAPGPU_SOLVER_DERIVE_PUBLIC; other keys keep their figures (their first _io call grows the scratch once).
 * LEFT OUT: a given form of the all-or-nothing capgpu_plonk_prove_batch /
 * _multi calls; a given form of capgpu_plonk_check_witness* (capgpu_plonk_solve_vars, then check); any hint kind beyond
 * the three; a rule that solves a row for two unknowns or inverts a product term; any change to the latency of ONE
 * witness's chain of dependent inversions (a lane-cooperative field product, another inversion algorithm). */
int capgpu_plonk_prove_given(const uint64_t* pk_handles, int count, const uint64_t* given, const uint64_t* pub_inputs,
                             size_t num_inputs, const uint8_t* const* ext_msgs, const size_t* ext_msg_lens,
                             const uint64_t* blinders, capgpu_proof* proofs_out, capgpu_prove_outcome* outcomes_out,
                             capgpu_solve_status* solved_out);
int capgpu_plonk_prove_given_dev(const uint64_t* pk_handles, int count, const void* d_given, const uint64_t* pub_inputs,
                                 size_t num_inputs, const uint8_t* const* ext_msgs, const size_t* ext_msg_lens,
                                 const uint64_t* blinders, capgpu_proof* proofs_out, capgpu_prove_outcome* outcomes_out,
                                 capgpu_solve_status* solved_out);
int capgpu_plonk_prove_given_async(const uint64_t* pk_handles, int count, const uint64_t* given, const uint64_t* pub_inputs,
                                   size_t num_inputs, const uint8_t* const* ext_msgs, const size_t* ext_msg_lens,
                                   const uint64_t* blinders, capgpu_proof* proofs_out, capgpu_prove_outcome* outcomes_out,
                                   capgpu_solve_status* solved_out, uint64_t* ticket_out);
int capgpu_plonk_prove_given_io(const uint64_t* pk_handles, int count, const uint64_t* given, size_t num_inputs,
                                const uint8_t* const* ext_msgs, const size_t* ext_msg_lens, const uint64_t* blinders,
                                uint64_t* pub_inputs_out, capgpu_proof* proofs_out, capgpu_prove_outcome* outcomes_out,
                                capgpu_solve_status* solved_out);
int capgpu_plonk_prove_given_io_dev(const uint64_t* pk_handles, int count, const void* d_given, size_t num_inputs,
                                    const uint8_t* const* ext_msgs, const size_t* ext_msg_lens, const uint64_t* blinders,
                                    uint64_t* pub_inputs_out, capgpu_proof* proofs_out, capgpu_prove_outcome* outcomes_out,
                                    capgpu_solve_status* solved_out);
int capgpu_plonk_prove_given_io_async(const uint64_t* pk_handles, int count, const uint64_t* given, size_t num_inputs,
                                      const uint8_t* const* ext_msgs, const size_t* ext_msg_lens, const uint64_t* blinders,
                                      uint64_t* pub_inputs_out, capgpu_proof* proofs_out,
                                      capgpu_prove_outcome* outcomes_out, capgpu_solve_status* solved_out,
                                      uint64_t* ticket_out);
int capgpu_plonk_reserve_given(uint64_t pk_handle, int count, int slot);
/* ONE PROOF PER CALL, GATHERED (capgpu_plonk_prove_given_one / _io_one): what a rayon worker holding one note's inputs
 * calls.  Outcome calls of one proof: CAPGPU_OK whenever the proof's batch ran, the verdict in outcome_out, an all-ones
 * record for a failed proof.  given holds the key's num_given values, pub_inputs (pub_inputs_out) its num_inputs; ext_msg
 * may be NULL with ext_msg_len 0; solved_out may be NULL.
 *   COALESCING OFF (the default): the call is capgpu_plonk_prove_given (_io) with count = 1.
 *   COALESCING ON (capgpu_plonk_set_coalescing): calls that arrive together are gathered as concurrent capgpu_plonk_prove
 *   calls are - same window, max_batch, in-flight limit and uneven cut over two contexts.  One group holds the given-value
 *   calls of one (domain size, SRS), all keys mixed; _io calls and plain calls form separate groups (a batch proves either
 *   against supplied or against computed public inputs), and neither ever shares a batch with wire-form capgpu_plonk_prove
 *   calls.  A gathered part packs its callers' rows in arrival order - given values and public inputs to the largest
 *   num_given / num_inputs among the part's keys, zeros behind a shorter row - and runs as ONE capgpu_plonk_prove_given
 *   (_io) call with a key per proof on the context the coalescer took: one staging copy, one solver launch per distinct
 *   key, witness check and compaction as that call applies them.  capgpu_plonk_coalescing_stats counts these batches and
 *   proofs with the others, capgpu_plonk_solve_stats the launches, capgpu_plonk_input_stats exactly 32 * num_given bytes
 *   per caller (the zero fill is the library's).
 *   THE CONTRACT.  proof_out, outcome_out, solved_out and - _io - pub_inputs_out are bit for bit what
 *   capgpu_plonk_prove_given (_io) with count = 1 writes for this caller's inputs alone in the same process modes
 *   (transcript home, wire commit, precheck, inverse form, solve form, solve pack), whichever other callers shared the
 *   batch and whatever their witnesses were.  One rule makes that so: with the witness check on, a lone refused witness
 *   returns after the check with degree_flags 0, while in an uncompacted batch it rides to the end and the degree check
 *   sets its flags as well - these calls report degree_flags = 0 for every outcome whose fault.kind != 0.
 *   REFUSALS, before a device is looked for: NULL given, blinders, proof_out or outcome_out, NULL pub_inputs
 *   (pub_inputs_out) with num_inputs > 0: CAPGPU_ERR_INVALID_ARG; then CAPGPU_ERR_NOT_INITIALISED; capgpu_plonk_shard_msm
 *   on: CAPGPU_ERR_INVALID_ARG.  num_given and num_inputs must be the key's: CAPGPU_ERR_INVALID_ARG
 *   ("capgpu_plonk_prove_given_one: 3 given values and 1 public inputs passed, the key has 4 and 1").
 *   FAILURES.  A request whose own key is gone (CAPGPU_ERR_BAD_HANDLE), has no solver or disagrees in num_given /
 *   num_inputs fails alone with its own code and message; the rest of its batch runs.  A failure of the part itself
 *   (CAPGPU_ERR_OOM, a HIP error) is returned to every caller of that part with that code and message.
 * LEFT OUT: a coalesced form over several domain sizes (one group is one domain size); pre-staging of the rows (a row is
 * a few KB); ticket and device-resident forms of the _one calls. */
int capgpu_plonk_prove_given_one(uint64_t pk_handle, const uint64_t* given, size_t num_given, const uint64_t* pub_inputs,
                                 size_t num_inputs, const uint8_t* ext_msg, size_t ext_msg_len, const uint64_t* blinders,
                                 capgpu_proof* proof_out, capgpu_prove_outcome* outcome_out,
                                 capgpu_solve_status* solved_out /* may be NULL */);
int capgpu_plonk_prove_given_io_one(uint64_t pk_handle, const uint64_t* given, size_t num_given, size_t num_inputs,
                                    const uint8_t* ext_msg, size_t ext_msg_len, const uint64_t* blinders,
                                    uint64_t* pub_inputs_out, capgpu_proof* proof_out, capgpu_prove_outcome* outcome_out,
                                    capgpu_solve_status* solved_out);

/* Batch compaction of the outcome calls (off by default; CAPGPU_COMPACT=1 sets the process default).  on != 0: an outcome
 * call made with capgpu_plonk_set_precheck on, of whose P witnesses the check refused some but not all, proves the P'
 * survivors as a batch of P' - every launch of the five rounds is that much smaller - and the refused ones cost their
 * check, not a proof.  A refused proof then has status CAPGPU_ERR_PROOF, its fault, an all-ones record and degree_flags
 * 0: it was never proved (uncompacted, the degree check sets its flags as well); status is still CAPGPU_ERR_PROOF exactly
 * when degree_flags != 0 || fault.kind != 0.  Surviving proofs are bit for bit the uncompacted call's.  The witness rows
 * of the survivors are brought together by one copy kernel ahead of round 1: in library staging (host-resident input,
 * variable form in either residence) at most min(bad, P') rows move; `_dev` columns and polynomials are the caller's
 * buffer, which is never written - the survivors' rows are copied into library staging when the proofs saved are worth
 * the copy (bad * 64 >= P'), and below that the call runs uncompacted.  What stays uncompacted besides: calls with the
 * witness check off (the degree check's verdict arrives in round 3, too late to be worth it), calls without outcomes,
 * coalesced capgpu_plonk_prove calls (gathered capgpu_plonk_prove_given_one parts are outcome calls and compact).  Dealt host batches and tickets compact per part.  Nothing changes while the mode is off.
 * Process-wide; read when a call - or a ticket - starts.  _get_: the mode in force.  _stats: counters since capgpu_init -
 * calls (parts of dealt calls) that ran compacted, proofs they dropped, witness rows handed to the copy kernel; any
 * pointer may be NULL. */
int capgpu_plonk_set_compaction(int on);
int capgpu_plonk_get_compaction(int* on_out);
int capgpu_plonk_compaction_stats(uint64_t* calls_out, uint64_t* proofs_dropped_out, uint64_t* rows_moved_out);
/* The message capgpu_plonk_prove_ex of that witness ALONE sets in the mode the outcome was made in: with a fault the
 * check's wording ("capgpu_plonk_prove: 1 of 1 witnesses do not satisfy their circuit; first: proof 0: gate 1234 not
 * satisfied" / "... proof 0: copy constraint (2,40) -> (0,7) violated"), otherwise the degree wording with `proof 0` and
 * the outcome's flags; an empty string for CAPGPU_OK.  At most cap - 1 characters and a NUL are written (cap 0: nothing).
 * Needs no device.  CAPGPU_ERR_INVALID_ARG for a NULL outcome, or a NULL buf with cap > 0. */
int capgpu_prove_outcome_text(const capgpu_prove_outcome* outcome, char* buf, size_t cap);

/* ---- verification (host only: needs neither a GPU nor capgpu_init) ---------------------------------------- */
/* G2 elements: x.c0, x.c1, y.c0, y.c1 of the twist point (Fq2 = Fq[u]/(u^2+1)), Montgomery, 16 words;
 * all-zero = infinity.  They are the `h` / `beta_h` of jf-plonk's VerifyingKey.open_key. */
int capgpu_g2_generator(uint64_t out[16]);
/* out = scalar * q (canonical 4 x u64 scalar): builds [tau]H for a synthetic SRS (src/proof/mod.rs:59-69) */
int capgpu_g2_mul(const uint64_t q[16], const uint64_t scalar[4], uint64_t out[16]);
/* *ok_out = (prod_i e(P_i, Q_i) == 1);  P_i: n affine G1 points (8 words each), Q_i: n G2 points (16 words each) */
int capgpu_pairing_check(const uint64_t* g1_points, const uint64_t* g2_points, size_t n, int* ok_out);
/* Replaces PlonkKzgSnark::verify::<SolidityTranscript> (src/proof/transfer.rs:192-212, mint.rs:124-140,
 * freeze.rs:162-178).  Returns CAPGPU_OK with *ok_out = 1 (accept) / 0 (reject); a negative code only for
 * malformed arguments (wrong number of public inputs, G2 elements off the curve). */
int capgpu_plonk_verify(const capgpu_verifying_key* vk, const uint64_t g2_h[16], const uint64_t g2_beta_h[16],
                        const uint64_t* pub_inputs, size_t num_inputs, const capgpu_proof* proof,
                        const uint8_t* ext_msg, size_t ext_msg_len, int* ok_out);

/* Replaces PlonkKzgSnark::batch_verify as used by txn_batch_verify (src/lib.rs:455-529): one pairing product for
 * `count` proofs (possibly of different circuits / keys under one SRS).  ext_msgs / ext_msg_lens may be NULL. */
int capgpu_plonk_batch_verify(const capgpu_verifying_key* const* vks, const uint64_t g2_h[16],
                              const uint64_t g2_beta_h[16], const uint64_t* const* pub_inputs,
                              const size_t* num_inputs, const capgpu_proof* const* proofs,
                              const uint8_t* const* ext_msgs, const size_t* ext_msg_lens, size_t count, int* ok_out);
/* The same predicate with its group arithmetic on the device: the ~35 (point, scalar) terms of every
 * proof, weights folded in, are two multi-scalar multiplications on the prover's MSM kernels (the bases are uploaded
 * like an SRS and their window tables built on the device); the transcripts and the final pairing product stay on the
 * host - the product too moves to the device, as one wave-form check, while the pairing form is CAPGPU_PAIRING_WAVE
 * (below).  Accepts and rejects exactly what capgpu_plonk_batch_verify does.  Needs capgpu_init
 * (CAPGPU_ERR_NOT_INITIALISED otherwise: no host path hides behind this entry point). */
int capgpu_plonk_batch_verify_dev(const capgpu_verifying_key* const* vks, const uint64_t g2_h[16],
                                  const uint64_t g2_beta_h[16], const uint64_t* const* pub_inputs,
                                  const size_t* num_inputs, const capgpu_proof* const* proofs,
                                  const uint8_t* const* ext_msgs, const size_t* ext_msg_lens, size_t count, int* ok_out);
/* ---- per-proof verification on the device (needs capgpu_init; CAPGPU_ERR_NOT_INITIALISED otherwise, no host path) --
 * Runs on the calling thread's bound context.  The pairing check is device code (Fq12 tower, Miller loop over prepared
 * lines of the two G2 points, final exponentiation: one check per lane). */
/* ok_out[i] = (e(p_i, q1) * e(r_i, q2) == 1) for i < count; p, r: count affine G1 points (8 words, Montgomery,
 * all-zero = infinity); q1, q2: twist points (16 words).  Off-curve input: CAPGPU_ERR_INVALID_ARG naming the index.
 * The two-pair, many-times form of capgpu_pairing_check (same verdict for each i). */
int capgpu_pairing_check_pairs_dev(const uint64_t* p, const uint64_t* r, size_t count, const uint64_t q1[16],
                                   const uint64_t q2[16], int* ok_out);
/* One verdict per proof, arguments as capgpu_plonk_batch_verify_dev; ok_out: count ints.  Replaces the loop of
 * TransferNote::verify (src/transfer.rs:345-363) that finds the bad notes of a block txn_batch_verify rejected:
 * ok_out[i] equals what capgpu_plonk_verify gives for proof i.  A proof that is off-curve, non-canonical, has zeta in
 * the domain or fails its pairing gets 0 and the call still returns CAPGPU_OK; negative codes only for the malformed
 * arguments capgpu_plonk_batch_verify rejects.  Transcripts and scalars on host threads; each proof's ~35 scalar
 * multiplications and its pairing check on the device. */
int capgpu_plonk_verify_each_dev(const capgpu_verifying_key* const* vks, const uint64_t g2_h[16],
                                 const uint64_t g2_beta_h[16], const uint64_t* const* pub_inputs,
                                 const size_t* num_inputs, const capgpu_proof* const* proofs,
                                 const uint8_t* const* ext_msgs, const size_t* ext_msg_lens, size_t count, int* ok_out);
/* ---- the pairing check's two forms ------------------------------------------------------------------------------
 * CAPGPU_PAIRING_LANE  one check per lane (k_pairing_check2): the throughput form.  Its duration is one lane's whole
 *                      pairing (~22 ms) for 1 check or for thousands.
 * CAPGPU_PAIRING_WAVE  one check per group of six lanes, ten per wavefront (k_pairing_check2_wave): meant for a
 *                      single proof or a small block; not yet timed against LANE.
 * The setting is process-wide, may be made before capgpu_init, starts as the environment's CAPGPU_PAIRING=lane|wave
 * (LANE when unset) and is honoured by capgpu_pairing_check_pairs_dev, capgpu_plonk_verify_each_dev and - for its
 * final pairing product, which LANE leaves on the host - capgpu_plonk_batch_verify_dev.  Verdicts do not depend on it.
 * An unknown value: CAPGPU_ERR_INVALID_ARG.  No reference counterpart (a scheduling choice of this library). */
#define CAPGPU_PAIRING_LANE 0
#define CAPGPU_PAIRING_WAVE 1
int capgpu_pairing_set_form(int form);
int capgpu_pairing_get_form(int* form_out);
/* Checks decided since process start by the lane-form and by the wave-form kernel (diagnostics: which path ran).
 * Either out pointer may be NULL. */
int capgpu_pairing_stats(uint64_t* lane_checks_out, uint64_t* wave_checks_out);
/* Replaces PlonkKzgSnark::verify::<SolidityTranscript> (proof::transfer::verify, src/proof/transfer.rs:192-212,
 * mint.rs:124-140, freeze.rs:162-178) for a caller that has a device: capgpu_plonk_verify's arguments (ext_msg before
 * proof here), the same range checks on every field word, the same verdict and return code in every case.  Transcript
 * and scalars on the host; the proof's ~35 scalar multiplications and its pairing check on the device, the check
 * always in the wave form whatever capgpu_pairing_set_form says.  Needs capgpu_init (CAPGPU_ERR_NOT_INITIALISED
 * otherwise: no host path hides behind this entry point). */
int capgpu_plonk_verify_dev(const capgpu_verifying_key* vk, const uint64_t g2_h[16], const uint64_t g2_beta_h[16],
                            const uint64_t* pub_inputs, size_t num_inputs, const uint8_t* ext_msg, size_t ext_msg_len,
                            const capgpu_proof* proof, int* ok_out);
/* ---- the block verifier: a whole block decided on the device, one host wait ------------------------------------------
 * Replaces txn_batch_verify (src/lib.rs:455-529) for a validator that replays blocks: each proof's transcript and its
 * ~35 scalars are derived by one wavefront (k_verify_front), the block is folded with 128-bit weights into two one-shot
 * MSMs (no window table) and one wave-form pairing check.  Only the preparation of the G2 lines of (beta_h, h) stays on
 * the host, and a context keeps the last pair's lines.
 *
 * capgpu_plonk_vk_upload checks a key once - domain_size a power of two >= 4, every point canonical and on the curve,
 * every k_i canonical; CAPGPU_ERR_INVALID_ARG names the field - and keeps its points, constants and transcript prefix
 * under a process-wide handle (needs no device; a context gets its copy on first use).  capgpu_plonk_vk_release drops it;
 * an unknown handle is CAPGPU_ERR_INVALID_ARG here and in the calls below.
 *
 * capgpu_plonk_verify_block_dev takes its arguments in capgpu_plonk_prove_multi's layouts: proofs one contiguous array,
 * pub_inputs `count` rows of num_inputs (at least the largest count among the call's keys; a key with fewer uses the
 * first of its row), ext_msgs / ext_msg_lens NULL or one entry per proof.  capgpu_plonk_verify_block_resident is the
 * same with d_pub_inputs and d_proofs in device memory (never written); the messages stay host arrays.
 *   *block_ok_out   the predicate of capgpu_plonk_batch_verify (up to the 2^-128 soundness of the weights);
 *   each_ok_out[i]  (NULL, or count ints) capgpu_plonk_verify's verdict for proof i, from the unweighted terms through
 *                   k_verify_terms and the pairing form in force, behind the block check and in the same wait.
 * block_ok == all(each_ok).  A bad proof (off-curve, non-canonical, zeta in the domain) gets 0 and never fails the call;
 * negative codes are for malformed arguments (unknown handle, num_inputs below a key's, G2 off the twist) and, after
 * those checks, CAPGPU_ERR_NOT_INITIALISED.  count == 0: *block_ok_out = 1.  Conventions of capgpu_msm_g1_var_dev: the
 * calling thread's context and stream, workspace from the context's scratch (capgpu_scratch_stats,
 * capgpu_set_memory_limit).  capgpu_verify_sync_stats: block calls that reached the device, and host waits on the stream
 * they made - one per call.  Either pointer may be NULL. */
int capgpu_plonk_vk_upload(const capgpu_verifying_key* vk, uint64_t* vk_handle_out);
int capgpu_plonk_vk_release(uint64_t vk_handle);
int capgpu_plonk_verify_block_dev(const uint64_t* vk_handles, const uint64_t g2_h[16], const uint64_t g2_beta_h[16],
                                  const uint64_t* pub_inputs, size_t num_inputs, const capgpu_proof* proofs,
                                  const uint8_t* const* ext_msgs, const size_t* ext_msg_lens, size_t count,
                                  int* block_ok_out, int* each_ok_out);
int capgpu_plonk_verify_block_resident(const uint64_t* vk_handles, const uint64_t g2_h[16], const uint64_t g2_beta_h[16],
                                       const void* d_pub_inputs, size_t num_inputs, const void* d_proofs,
                                       const uint8_t* const* ext_msgs, const size_t* ext_msg_lens, size_t count,
                                       int* block_ok_out, int* each_ok_out);
int capgpu_verify_sync_stats(uint64_t* block_calls_out, uint64_t* stream_waits_out);
/* ark-serialize 0.3 CanonicalSerialize bytes of the Proof as it sits inside a TransferNote / MintNote / FreezeNote
 * (src/transfer.rs:60): compressed G1 (32 B), Fr little-endian, Vec = u64 length prefix, plookup_proof = None.
 * 769 bytes; *len_out receives the size. */
int capgpu_proof_serialize(const capgpu_proof* proof, uint8_t* out, size_t cap, size_t* len_out);
/* The inverse (`Proof::deserialize`, what reading a note from bytes does): CAPGPU_ERR_SERIALIZATION on every encoding
 * ark-serialize rejects (vector lengths, non-canonical x or scalar, x off the curve, both flag bits, a plookup
 * proof).  Host only.  *consumed_out receives the bytes read. */
int capgpu_proof_deserialize(const uint8_t* bytes, size_t len, capgpu_proof* proof_out, size_t* consumed_out);

/* ---- proofs as note bytes, in bulk and on the device ------------------------------------------------------------------
 * A validator holds a proof as the 769 bytes above, never as a capgpu_proof.  These calls run the rule of
 * capgpu_proof_deserialize / capgpu_proof_serialize on the device for a whole block (k_proof_decode: one lane per
 * compressed point, whole wavefronts on the square-root chain; k_proof_encode), and the two _bytes verifiers below take
 * a block from note bytes to verdicts with one host wait.
 *
 * Records: `count` of them, record i at bytes + i * stride, stride >= CAPGPU_PROOF_BYTES, any byte address (nothing is
 * read wider than a byte); the bytes between records are neither read nor written.
 *   status_out[i]  0 for a record capgpu_proof_deserialize accepts, else 1 + the byte offset of the first field it
 *                  would have stopped at: a length prefix (0, 200, 432, 600), a compressed point (8 + 32 k, 168,
 *                  208 + 32 k, 368, 400), an evaluation (440 + 32 k, 608 + 32 k, 736) or the Option tag (768).
 *   proofs_out[i]  the decoded proof, word for word capgpu_proof_deserialize's; for a record whose status is not 0
 *                  every word is 0xFFFFFFFFFFFFFFFF - no coordinate or evaluation of it is canonical, so every verifier
 *                  of this library rejects it by its own range checks.
 * A malformed record never fails a call: CAPGPU_OK whatever the records hold.  stride < CAPGPU_PROOF_BYTES, a null
 * pointer with count > 0 or count > 2^24: CAPGPU_ERR_INVALID_ARG before a device is looked for; count == 0 is CAPGPU_OK
 * (after CAPGPU_ERR_NOT_INITIALISED). */
#define CAPGPU_PROOF_BYTES 769
/* Replaces a loop of capgpu_proof_deserialize (Proof::deserialize per note, 13 square roots in Fq each on one host
 * thread): host buffers, one upload, one launch sequence, one wait. */
int capgpu_proof_decode_batch(const uint8_t* bytes, size_t stride, size_t count, capgpu_proof* proofs_out, int* status_out);
/* The same on device buffers (d_proofs_out 16-byte aligned, d_status_out 4-byte aligned): enqueued on the calling
 * context's stream, no wait - the conventions of capgpu_msm_g1_var_dev. */
int capgpu_proof_decode_batch_dev(const void* d_bytes, size_t stride, size_t count, void* d_proofs_out, int* d_status_out);
/* Replaces a loop of capgpu_proof_serialize: record i receives exactly its bytes for proofs[i] (the inverse of the
 * decoder on canonical proofs).  _dev: device buffers, enqueued, no wait - a prover's proofs become note bytes without
 * leaving the device. */
int capgpu_proof_encode_batch(const capgpu_proof* proofs, size_t count, uint8_t* bytes_out, size_t stride);
int capgpu_proof_encode_batch_dev(const void* d_proofs, size_t count, void* d_bytes_out, size_t stride);
/* capgpu_plonk_verify_block_dev / capgpu_plonk_verify_block_resident with the proofs given as note bytes (replaces a loop
 * of capgpu_proof_deserialize in front of them): the records are decoded into the call's scratch and the block
 * verifier's launch sequence runs on that buffer.  decode_status_out: NULL or count ints, the statuses above.
 * each_ok_out[i] = (status i == 0) && capgpu_plonk_verify's verdict on the decoded proof; *block_ok_out == all(each_ok).
 * A malformed record never fails the call.  Still one stream wait per call (capgpu_verify_sync_stats); workspace from
 * the context's scratch.  _resident: d_pub_inputs and d_proof_bytes in device memory, never written. */
int capgpu_plonk_verify_block_bytes(const uint64_t* vk_handles, const uint64_t g2_h[16], const uint64_t g2_beta_h[16],
                                    const uint64_t* pub_inputs, size_t num_inputs, const uint8_t* proof_bytes,
                                    size_t stride, const uint8_t* const* ext_msgs, const size_t* ext_msg_lens,
                                    size_t count, int* block_ok_out, int* each_ok_out, int* decode_status_out);
int capgpu_plonk_verify_block_bytes_resident(const uint64_t* vk_handles, const uint64_t g2_h[16],
                                             const uint64_t g2_beta_h[16], const void* d_pub_inputs, size_t num_inputs,
                                             const void* d_proof_bytes, size_t stride, const uint8_t* const* ext_msgs,
                                             const size_t* ext_msg_lens, size_t count, int* block_ok_out,
                                             int* each_ok_out, int* decode_status_out);

/* ---- on-disk parameter formats ------------------------------------------------------
 * The reference stores and loads its parameters as ark-serialize 0.3 `CanonicalSerialize` bytes
 * (store_data / load_data, src/parameters.rs:560-577; load_srs, src/proof/mod.rs:74-109) and notes that
 * "deserializing these parameter files takes longer than reproducing them" (src/lib.rs:81-86): the cost is a
 * square root in Fq per compressed point.  Here the bulk G1 decompression is one kernel launch.
 * Encodings: usize = u64 LE; Vec / BTreeMap = u64 length + items; Fr = 32 B LE canonical; G1 compressed = x (32 B
 * LE) with 0x80 of the last byte = "y is the larger root" and 0x40 = infinity; G2 compressed = x.c0, x.c1 (64 B)
 * with the same flags in the last byte.  The field order inside each struct is restated from the crates'
 * definitions (ark-poly-commit @ cafc05e, jf-plonk @ bcd92b2), which are not in the reference tree: parity with a
 * blob written by the reference is unpinned. */

/* n compressed G1 points (32 B each) <-> affine (x, y), 8 Montgomery words each, (0, 0) = infinity.
 * Decompression fails with CAPGPU_ERR_SERIALIZATION on x >= p, x not on the curve, or both flag bits set. */
int capgpu_g1_decompress(const uint8_t* in, size_t n, uint64_t* out_xy);
int capgpu_g1_compress(const uint64_t* xy, size_t n, uint8_t* out);

/* UniversalSrs blob (parameters::load_universal_parameter, src/parameters.rs:97-109; load_srs): validates every
 * point, keeps the first max_degree + 1 powers of g resident (0 = all) and returns the handle plus the open key
 * (h, beta_h: G2 affine, x.c0 x.c1 y.c0 y.c1 Montgomery).  *consumed_out = bytes read. */
int capgpu_srs_deserialize(const uint8_t* bytes, size_t len, size_t max_degree, uint64_t* handle_out,
                           uint64_t h_out[16], uint64_t beta_h_out[16], size_t* consumed_out);
/* parameters::store_universal_parameter_for_demo (src/parameters.rs:47-65).  out == NULL queries the size. */
int capgpu_srs_serialize(uint64_t handle, const uint64_t h[16], const uint64_t beta_h[16], uint8_t* out, size_t cap,
                         size_t* len_out);

/* jf-plonk VerifyingKey blob (store_/load_*_verifying_key, src/parameters.rs:190-241, 314-362, 438-478) without
 * the note-shape trailer the Transfer/Mint/Freeze wrappers append (src/proof/transfer.rs:83-94); host only.
 * g, gamma_g: the G1 part of the open key (gamma_g may be NULL on serialize = infinity: commitments here are
 * non-hiding and neither prover nor verifier reads it).  capgpu_plonk_key_serialize with gamma_g == NULL writes the
 * gamma_g of the blob the key - or the UniversalSrs it was preprocessed under (degree 0 of its hiding powers) - was
 * loaded from, so that load -> store gives the file back; infinity for a synthetic SRS. */
int capgpu_plonk_vk_serialize(const capgpu_verifying_key* vk, const uint64_t g[8], const uint64_t gamma_g[8],
                              const uint64_t h[16], const uint64_t beta_h[16], uint8_t* out, size_t cap,
                              size_t* len_out);
int capgpu_plonk_vk_deserialize(const uint8_t* bytes, size_t len, capgpu_verifying_key* vk_out, uint64_t g_out[8],
                                uint64_t gamma_g_out[8], uint64_t h_out[16], uint64_t beta_h_out[16],
                                size_t* consumed_out);

/* jf-plonk ProvingKey blob (store_/load_*_proving_key, src/parameters.rs:113-188, 244-312, 364-436), again without
 * the wrapper's trailer: sigma and selector polynomials, the commit key and the verifying key.  Deserialising
 * decompresses the commit key on the device, registers it as a new SRS (*srs_handle_out, owned by the caller) and
 * rebuilds the resident tables of the prover without redoing the 18 interpolations and commitments of
 * preprocess.  out == NULL on serialize queries the size. */
int capgpu_plonk_key_serialize(uint64_t pk_handle, const uint64_t gamma_g[8], const uint64_t h[16],
                               const uint64_t beta_h[16], uint8_t* out, size_t cap, size_t* len_out);
int capgpu_plonk_key_deserialize(const uint8_t* bytes, size_t len, uint64_t* srs_handle_out, uint64_t* pk_handle_out,
                                 capgpu_verifying_key* vk_out, uint64_t h_out[16], uint64_t beta_h_out[16],
                                 size_t* consumed_out);

/* ---- parameter audit: look at an SRS and a proving key before trusting them (needs capgpu_init; no host path) ----------
 * The reference guards its ceremony file with a SHA-256 over the bytes before it deserialises (load_srs,
 * src/proof/mod.rs:95-102) and reads its key files with no check at all (load_data, src/parameters.rs:560-577).  A wrong,
 * truncated or swapped point, a beta_h from another ceremony or a key file whose polynomials do not match its commitments
 * all give proofs no verifier accepts, and nothing on the proving side says why.  These two calls ask the questions a hash
 * cannot: call them ONCE per loaded file, not per proof.
 * Conventions of capgpu_plonk_check_witness*: CAPGPU_OK whenever the check RAN - the verdict is in the report; the same
 * inputs (and seed) give the same report on every run; negative codes are for malformed arguments only (out == NULL,
 * unknown flag bits, G2 input off the twist or at infinity - all refused before a device is looked for - and an unknown
 * handle), CAPGPU_ERR_NOT_INITIALISED before capgpu_init.  Both run on the calling thread's context and stream
 * (capgpu_set_stream is honoured) and take their workspace from the context's scratch (capgpu_scratch_stats counts it,
 * capgpu_set_memory_limit caps it: CAPGPU_ERR_OOM naming the bytes).
 *
 * capgpu_srs_check: are the resident points P[0 .. n) of the handle a power sequence P[i + 1] = tau P[i] for the tau of the
 * open key (h, beta_h = [tau] h)?
 *   a. point pass: every P[i] is on y^2 = x^3 + 3 and not infinity (capgpu_srs_upload does not check this); a fault ends
 *      the call with verdict 1 - the fold is not run on what is no group element (pairing_checks = 0);
 *   b. weights r_i, i < n - 1: the first 16 bytes, little-endian, of Keccak-256(seed || le64(i)) (the block verifier's
 *      byte convention; every i is hashed);
 *   c. fold: A = sum r_i P[i], B = sum r_i P[i + 1] - two MSMs over the same weights on the resident table;
 *   d. e(A, beta_h) e(-B, h) == 1 by one wave-form pairing check on the device; failure is verdict 2;
 *   e. CAPGPU_SRS_CHECK_LOCATE, after a verdict 2 only: bisection on the prefix length k - the prefix [0, k] passes iff
 *      sum_{i<k} r_i P[i] and sum_{i<k} r_i P[i + 1] pair up - finds the lowest bad link in at most ceil(log2 n) rounds.
 * The call waits for the device once, and once more per bisection round.  n == 1 has no links: verdict 0, no pairing.
 * Soundness: a consistent SRS is ALWAYS accepted (B = tau A exactly); an inconsistent one is accepted with probability
 * about 2^-128 over a seed its author did not know - hence seed == NULL draws 32 bytes from the operating system, and a
 * caller-given seed is for reproducibility.  Not covered: the hiding powers (powers_of_gamma_g: host-side bytes the prover
 * never reads), neg_powers_of_h, whether P[0] is any particular generator, and the window tables the library derives
 * itself from the points.  A sharded SRS is refused (CAPGPU_ERR_INVALID_ARG). */
#define CAPGPU_SRS_CHECK_LOCATE 1u   /* on a structure fault, find the first bad link (bisection) */
typedef struct capgpu_srs_report {
  uint32_t verdict;          /* 0 consistent, 1 point fault, 2 structure fault */
  uint32_t point_fault;      /* 0 none, 1 a point at infinity, 2 a point off the curve */
  uint64_t first_bad_point;  /* verdict 1: lowest index with a point fault; else UINT64_MAX */
  uint64_t first_bad_link;   /* verdict 2 with LOCATE: lowest i with P[i+1] != tau P[i]; else UINT64_MAX */
  uint64_t points_checked, links_checked;   /* n and n - 1 (0 links when a point fault ended the call) */
  uint32_t pairing_checks;   /* 1, or 1 + the bisection's rounds; 0 when no fold was made */
  uint32_t reserved;
  uint64_t fold_a[8], fold_b[8];  /* A = sum r_i P[i], B = sum r_i P[i+1], i < n-1: affine, Montgomery, (0,0) = infinity */
} capgpu_srs_report;          /* 176 bytes */
int capgpu_srs_check(uint64_t srs_handle, const uint64_t g2_h[16], const uint64_t g2_beta_h[16],
                     const uint8_t seed[32] /* NULL: drawn from the OS */, uint32_t flags, capgpu_srs_report* out);
/* capgpu_plonk_key_check: does this proving key produce this verifying key?  capgpu_plonk_key_deserialize "rebuilds the
 * resident tables of the prover without redoing the 18 interpolations and commitments of preprocess": the verifying key
 * inside a proving-key blob is taken on faith.  This call commits to the key's 18 polynomials again (one batched MSM on
 * the key's SRS), compares the affine commitments word for word with vk's, compares domain_size, num_inputs and k[], and
 * runs the witness check's test that sigma's values lie in the five cosets k_i H.  vk == NULL: the key's own verifying
 * key - the check to run after capgpu_plonk_key_deserialize.  When several faults are present the lowest verdict is
 * reported. */
typedef struct capgpu_key_report {
  uint32_t verdict;      /* 0 consistent, 1 shape (domain_size / num_inputs / k differ), 2 commitment differs, 3 sigma is no permutation */
  uint32_t column;       /* verdict 2: 0..12 selector (gate order of capgpu_verifying_key), 13..17 sigma; lowest differing */
  uint32_t columns_differing, reserved;
} capgpu_key_report;     /* 16 bytes */
int capgpu_plonk_key_check(uint64_t pk_handle, const capgpu_verifying_key* vk /* NULL: the key's own */,
                           capgpu_key_report* out);

/* ---- instrumentation ------------------------------------------------------------------------------ */
/* Measured issue rate of v_mad_u64_u32 on the bound device, in lane-operations per second (8 independent chains per
 * lane, 8 waves per SIMD, ~50 ms).  A lazy Montgomery multiplication is 171 of them (81 + 81 + 9), so rate / 171 is the
 * chip's multiplication ceiling - what bench.py prices the ALU-bound kernels against. */
int capgpu_ubench_mad_rate(double* lane_ops_per_s_out);
/* The same measurement for the instruction classes the hot kernels are made of, all at that occupancy and chain count,
 * in lane-operations per second: rates_out[0..count) = v_mad_u64_u32, v_add_u32, v_and_b32, v_mov_b32, v_lshl_add_u64,
 * v_lshrrev_b64, v_alignbit_b32, v_mul_lo_u32, then [8] a mixed stream - three multiply-adds, one plain instruction, the
 * shape of a column-wise Montgomery product - at the same occupancy and [9] the same stream held to three waves per SIMD,
 * msm_accumulate's occupancy (count <= 10; ~0.4 s).  bench.py prices a kernel's instruction mix
 * (profiles/isa_mix_r03.json) against them: issue_frac. */
int capgpu_ubench_issue_rates(double* rates_out, int count);
/* When enabled, every kernel launch is bracketed by HIP events on the launch stream and accumulated
 * per kernel name (costs a few microseconds per launch; leave off for throughput runs). */
int capgpu_profile_enable(int on);
int capgpu_profile_reset(void);
/* name == kernel name (e.g. "msm_accumulate"); total milliseconds and launch count since reset */
int capgpu_profile_get(const char* name, double* total_ms_out, uint64_t* launches_out);
/* writes up to cap bytes of "name total_ms launches\n" lines */
int capgpu_profile_dump(char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* CAPGPU_H */
