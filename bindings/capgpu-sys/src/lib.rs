//! Raw bindings of `include/capgpu.h` (libcapgpu.so, the MI355X PLONK prover) and the thin safe layer above them.
//!
//! UNBUILT in this repository (no Rust toolchain there); see Cargo.toml.  The `extern "C"` block mirrors the header
//! symbol for symbol - integers little-endian, `Fr`/`Fq` = `[u64; 4]` (arkworks `BigInteger256` limb order, Montgomery
//! form where the header says so), G1 affine = 8 words, G1 Jacobian = 12 words, G2 affine = 16 words.  Every function
//! returns `CAPGPU_OK` (0) or a negative `CAPGPU_ERR_*`; nothing unwinds across the boundary.
//!
//! Replaces, in the reference (EspressoSystems/cap):
//!   `PlonkKzgSnark::preprocess` at src/proof/transfer.rs:133, mint.rs:76, freeze.rs:102   -> `ProvingKey::preprocess`
//!   `PlonkKzgSnark::prove`      at src/proof/transfer.rs:181-186, mint.rs:113, freeze.rs:151 -> `ProvingKey::prove`
//!   `VariableBaseMSM::multi_scalar_mul` (ark-ec 0.3.0, via KZG10::commit)                  -> `Srs::msm`
//!   `Radix2EvaluationDomain::{fft,ifft,coset_fft,coset_ifft}_in_place` (ark-poly 0.3.0)    -> `ntt_in_place`
#![allow(non_camel_case_types)]

use std::os::raw::{c_char, c_int, c_void};

pub const CAPGPU_OK: c_int = 0;
pub const CAPGPU_ERR_INVALID_ARG: c_int = -1;
pub const CAPGPU_ERR_NO_DEVICE: c_int = -2;
pub const CAPGPU_ERR_HIP: c_int = -3;
pub const CAPGPU_ERR_BAD_HANDLE: c_int = -4;
pub const CAPGPU_ERR_OOM: c_int = -5;
pub const CAPGPU_ERR_NOT_INITIALISED: c_int = -6;
pub const CAPGPU_ERR_PROOF: c_int = -7;
pub const CAPGPU_ERR_SERIALIZATION: c_int = -8;
pub const CAPGPU_ERR_COMM: c_int = -9;
pub const CAPGPU_ERR_BUSY: c_int = -10;

pub const NUM_WIRE_TYPES: usize = 5;
pub const NUM_SELECTORS: usize = 13;

/// `input_form` of the `_ex` PLONK entry points: values on the domain, or polynomials in coefficient form - what
/// jf-relation's `Arithmetization` trait returns, passed through without a CPU transform.
pub const CAPGPU_INPUT_EVALS: c_int = 0;
pub const CAPGPU_INPUT_COEFFS: c_int = 1;
pub const CAPGPU_INPUT_VARS: c_int = 2;

/// `capgpu_proof`: the fields of `jf_plonk::proof_system::structs::Proof`, in order (plookup_proof = None).
#[repr(C)]
#[derive(Clone, Copy)]
pub struct capgpu_proof {
    pub wires_poly_comms: [[u64; 8]; NUM_WIRE_TYPES],
    pub prod_perm_poly_comm: [u64; 8],
    pub split_quot_poly_comms: [[u64; 8]; NUM_WIRE_TYPES],
    pub opening_proof: [u64; 8],
    pub shifted_opening_proof: [u64; 8],
    pub wires_evals: [[u64; 4]; NUM_WIRE_TYPES],
    pub wire_sigma_evals: [[u64; 4]; NUM_WIRE_TYPES - 1],
    pub perm_next_eval: [u64; 4],
}

/// `capgpu_verifying_key`: `jf_plonk::proof_system::structs::VerifyingKey` without the open key.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct capgpu_verifying_key {
    pub domain_size: u64,
    pub num_inputs: u64,
    pub k: [[u64; 4]; NUM_WIRE_TYPES],
    pub selector_comms: [[u64; 8]; NUM_SELECTORS],
    pub sigma_comms: [[u64; 8]; NUM_WIRE_TYPES],
}

/// `capgpu_ntt_plan_info`: how `capgpu_ntt_plan` says a transform is launched (72 bytes); one entry per pass in the
/// order the passes run, the row pass last.
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct capgpu_ntt_plan_info {
    pub passes: u32,
    pub tile_log: u32,
    pub digits: [u32; 3],
    pub log_c: [u32; 3],
    pub tiles: [u64; 3],
    pub persistent: [u32; 3],
    pub reserved: u32,
}

/// `capgpu_witness_fault`: the verdict of the witness check for one proof (48 bytes).
/// `kind`: 0 satisfied, 1 gate `row`, 2 copy constraint `(wire, row) -> (wire2, row2)`.
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct capgpu_witness_fault {
    pub kind: u32,
    pub wire: u32,
    pub wire2: u32,
    pub reserved: u32,
    pub row: u64,
    pub row2: u64,
    pub gates_failed: u64,
    pub copies_failed: u64,
}

/// `capgpu_solver_info`: the figures of a key's witness-solver schedule (48 bytes); all zero: the key has no solver.
#[repr(C)]
#[derive(Clone, Copy, Default, Debug, PartialEq, Eq)]
pub struct capgpu_solver_info {
    pub num_given: u64,
    pub num_defined: u64,
    pub levels: u64,
    pub widest_level: u64,
    pub inv_rows: u64,
    pub root_rows: u64,
}

/// `capgpu_hint`: one solver hint (16 bytes): `count` targets, `targets[first .. first + count)`, valued from `src`.
#[repr(C)]
#[derive(Clone, Copy, Default, Debug, PartialEq, Eq)]
pub struct capgpu_hint {
    pub kind: u32,
    pub src: u32,
    pub first: u32,
    pub count: u32,
}
pub const CAPGPU_HINT_BITS: u32 = 0;
pub const CAPGPU_HINT_INV0: u32 = 1;
pub const CAPGPU_HINT_ISZERO: u32 = 2;

/// `capgpu_hint_info`: the figures of a key's solver hints (48 bytes); all zero: the key has none.
#[repr(C)]
#[derive(Clone, Copy, Default, Debug, PartialEq, Eq)]
pub struct capgpu_hint_info {
    pub num_hints: u64,
    pub num_hinted: u64,
    pub bits_hints: u64,
    pub inv_hints: u64,
    pub iszero_hints: u64,
    pub hint_items: u64,
}

/// `capgpu_solver_rules_info`: the flags a key's solver was set with (`capgpu_plonk_key_set_solver`), its LIN rows and the
/// public-input rows whose variable the solver derives (32 bytes); all zero: no solver.
#[repr(C)]
#[derive(Clone, Copy, Default, Debug, PartialEq, Eq)]
pub struct capgpu_solver_rules_info {
    pub flags: u64,
    pub lin_rows: u64,
    pub derived_inputs: u64,
    pub reserved: u64,
}
pub const CAPGPU_SOLVER_LINEAR: u32 = 1;
pub const CAPGPU_SOLVER_DERIVE_PUBLIC: u32 = 2;

/// `capgpu_solve_form_info`: the form of the schedule a key's solver runs (`capgpu_plonk_key_set_solve_form`) and its
/// figures (64 bytes); all zero: no solver.
#[repr(C)]
#[derive(Clone, Copy, Default, Debug, PartialEq, Eq)]
pub struct capgpu_solve_form_info {
    pub form: u64,
    pub deferred_vars: u64,
    pub frac_rows: u64,
    pub flush_levels: u64,
    pub flush_items: u64,
    pub levels: u64,
    pub inv_levels_direct: u64,
    pub inv_levels_deferred: u64,
}
pub const CAPGPU_SOLVE_FORM_DIRECT: c_int = 0;
pub const CAPGPU_SOLVE_FORM_DEFERRED: c_int = 1;

/// `capgpu_solve_status`: the verdict of the witness solver for one witness (16 bytes).  `kind`: 0 solved, 1 the
/// denominator of `row` - the lowest such row - is zero (its variable is 0).
#[repr(C)]
#[derive(Clone, Copy, Default, Debug, PartialEq, Eq)]
pub struct capgpu_solve_status {
    pub kind: u32,
    pub reserved: u32,
    pub row: u64,
}

/// `capgpu_prove_outcome`: the verdict of one proof of a `capgpu_plonk_prove_each*` call (56 bytes).  `status` is
/// `CAPGPU_ERR_PROOF` exactly when `degree_flags != 0 || fault.kind != 0`; the record of such a proof is all-ones words.
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct capgpu_prove_outcome {
    pub status: i32,
    pub degree_flags: u32,
    pub fault: capgpu_witness_fault,
}

/// `capgpu_notes_group`: one group of a `capgpu_plonk_prove_notes*` call - the notes whose keys share domain size and SRS
/// (32 bytes).  `first`: its lowest note index; `run_order` 0 starts first.
#[repr(C)]
#[derive(Clone, Copy, Default, Debug, PartialEq, Eq)]
pub struct capgpu_notes_group {
    pub srs_handle: u64,
    pub domain_size: u64,
    pub count: u32,
    pub first: u32,
    pub max_inputs: u32,
    pub run_order: u32,
}

/// `capgpu_notes_stats`: process-wide counters of the notes calls since `capgpu_init` (56 bytes).
#[repr(C)]
#[derive(Clone, Copy, Default, Debug, PartialEq, Eq)]
pub struct capgpu_notes_stats {
    pub calls: u64,
    pub groups: u64,
    pub groups_dealt: u64,
    pub contexts_dealt: u64,
    pub dev_groups_direct: u64,
    pub dev_groups_gathered: u64,
    pub rows_gathered: u64,
}

/// `flags` of `capgpu_srs_check`: on a structure fault, find the first bad link by bisection.
pub const CAPGPU_SRS_CHECK_LOCATE: u32 = 1;

/// `capgpu_srs_report`: the verdict of `capgpu_srs_check` (176 bytes).  `verdict`: 0 consistent, 1 point fault
/// (`point_fault`: 1 infinity, 2 off the curve, at `first_bad_point`), 2 structure fault (`first_bad_link` with LOCATE).
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct capgpu_srs_report {
    pub verdict: u32,
    pub point_fault: u32,
    pub first_bad_point: u64,
    pub first_bad_link: u64,
    pub points_checked: u64,
    pub links_checked: u64,
    pub pairing_checks: u32,
    pub reserved: u32,
    pub fold_a: [u64; 8],
    pub fold_b: [u64; 8],
}

/// `capgpu_key_report`: the verdict of `capgpu_plonk_key_check` (16 bytes).  `verdict`: 0 consistent, 1 shape, 2 a
/// commitment differs (`column`: 0..12 selector, 13..17 sigma), 3 sigma is no permutation.
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct capgpu_key_report {
    pub verdict: u32,
    pub column: u32,
    pub columns_differing: u32,
    pub reserved: u32,
}

#[link(name = "capgpu")]
extern "C" {
    // ---- lifecycle, devices
    pub fn capgpu_init(device_ids: *const c_int, n_devices: c_int) -> c_int;
    pub fn capgpu_shutdown();
    pub fn capgpu_last_error() -> *const c_char;
    pub fn capgpu_version() -> *const c_char;
    pub fn capgpu_device_count(count_out: *mut c_int) -> c_int;
    pub fn capgpu_set_device(slot: c_int) -> c_int;
    pub fn capgpu_get_device(slot_out: *mut c_int, hip_device_out: *mut c_int) -> c_int;
    pub fn capgpu_device_info(name_out: *mut c_char, cu_count_out: *mut c_int, hbm_bytes_out: *mut u64) -> c_int;
    pub fn capgpu_device_peer_info(slot_a: c_int, slot_b: c_int, access_out: *mut c_int) -> c_int;
    pub fn capgpu_mem_info(free_bytes_out: *mut u64, total_bytes_out: *mut u64) -> c_int;
    // ---- footprint control and diagnostics
    pub fn capgpu_trim(bytes_released_out: *mut u64, contexts_busy_out: *mut c_int) -> c_int;
    pub fn capgpu_set_memory_limit(scratch_bytes_per_device: u64) -> c_int;
    pub fn capgpu_scratch_info(scratch_bytes_out: *mut u64, limit_out: *mut u64) -> c_int;
    pub fn capgpu_scratch_stats(grow_events_out: *mut u64, grow_bytes_out: *mut u64, grow_ms_out: *mut f64) -> c_int;
    pub fn capgpu_trace_enable(on: c_int) -> c_int;
    pub fn capgpu_trace_dump(path: *const c_char, events_out: *mut u64) -> c_int;
    // ---- device memory / stream
    pub fn capgpu_malloc(dev_ptr_out: *mut *mut c_void, bytes: usize) -> c_int;
    pub fn capgpu_free(dev_ptr: *mut c_void) -> c_int;
    pub fn capgpu_memcpy_h2d(dev_dst: *mut c_void, host_src: *const c_void, bytes: usize) -> c_int;
    pub fn capgpu_memcpy_d2h(host_dst: *mut c_void, dev_src: *const c_void, bytes: usize) -> c_int;
    pub fn capgpu_sync() -> c_int;
    pub fn capgpu_sync_all() -> c_int;
    pub fn capgpu_runtime_info(hip_runtime_version_out: *mut c_int, hip_driver_version_out: *mut c_int) -> c_int;
    pub fn capgpu_timer_begin() -> c_int;
    pub fn capgpu_timer_end(ms_out: *mut f64) -> c_int;
    pub fn capgpu_context_count(count_out: *mut c_int) -> c_int;
    pub fn capgpu_physical_device_count(count_out: *mut c_int) -> c_int;
    pub fn capgpu_set_stream(hip_stream: *mut c_void) -> c_int;
    // ---- SRS
    pub fn capgpu_srs_upload(bases: *const c_void, n: usize, stride_bytes: usize, coords_montgomery: c_int,
                             handle_out: *mut u64) -> c_int;
    pub fn capgpu_srs_generate(tau: *const u64, n: usize, handle_out: *mut u64) -> c_int;
    pub fn capgpu_srs_generate_hiding(tau: *const u64, gamma: *const u64, n: usize, handle_out: *mut u64) -> c_int;
    pub fn capgpu_srs_generate_affine_seq(a: *const u64, b: *const u64, n: usize, handle_out: *mut u64) -> c_int;
    pub fn capgpu_srs_size(handle: u64, n_out: *mut usize) -> c_int;
    pub fn capgpu_srs_shards(handle: u64, shards_out: *mut c_int) -> c_int;
    pub fn capgpu_srs_download(handle: u64, offset: usize, n: usize, out: *mut c_void) -> c_int;
    pub fn capgpu_srs_free(handle: u64) -> c_int;
    // ---- MSM
    pub fn capgpu_msm_g1(srs_handle: u64, offset: usize, scalars: *const u64, n: usize, out_xyz: *mut u64) -> c_int;
    pub fn capgpu_msm_g1_lagrange(
        srs_handle: u64,
        log_n: u32,
        scalars: *const u64,
        count: usize,
        scalars_montgomery: c_int,
        out_xyz: *mut u64,
    ) -> c_int;
    pub fn capgpu_msm_g1_batch(srs_handle: u64, offsets: *const usize, scalars: *const *const u64, ns: *const usize,
                               count: c_int, out_xyz: *mut u64) -> c_int;
    pub fn capgpu_msm_g1_dev(srs_handle: u64, offset: usize, d_scalars: *const c_void, scalar_stride: usize, n: usize,
                             count: c_int, scalars_montgomery: c_int, d_out_xyz: *mut c_void) -> c_int;
    pub fn capgpu_msm_scalars_upload(srs_handle: u64, offset: usize, scalars: *const u64, scalar_stride: usize, n: usize,
                                     count: c_int, scalars_handle_out: *mut u64) -> c_int;
    pub fn capgpu_msm_scalars_scatter_dev(srs_handle: u64, offset: usize, d_scalars: *const c_void, scalar_stride: usize,
                                          n: usize, count: c_int, scalars_handle_out: *mut u64) -> c_int;
    pub fn capgpu_msm_scalars_free(scalars_handle: u64) -> c_int;
    pub fn capgpu_msm_g1_resident(srs_handle: u64, scalars_handle: u64, scalars_montgomery: c_int,
                                  d_out_xyz: *mut c_void) -> c_int;
    pub fn capgpu_msm_shard_stats(scalar_bytes_out: *mut u64, partial_bytes_out: *mut u64, calls_out: *mut u64,
                                  replications_out: *mut u64) -> c_int;
    pub fn capgpu_msm_plan(srs_handle: u64, n: usize, count: c_int, buf: *mut c_char, cap: usize) -> c_int;
    pub fn capgpu_msm_tail_plan(c: c_int, n_sub: usize, sub_msms: c_int, has_parts: c_int, buf: *mut c_char,
                                cap: usize) -> c_int;
    // ---- one-shot MSM over caller points (no handle, no table)
    pub fn capgpu_msm_g1_var(bases: *const c_void, stride_bytes: usize, coords_montgomery: c_int, scalars: *const u64,
                             n: usize, out_xyz: *mut u64) -> c_int;
    pub fn capgpu_msm_g1_var_batch(bases: *const *const u64, scalars: *const *const u64, ns: *const usize, count: c_int,
                                   out_xyz: *mut u64) -> c_int;
    pub fn capgpu_msm_g1_var_dev(d_bases: *const c_void, d_scalars: *const c_void, scalar_stride: usize, n: usize,
                                 count: c_int, scalars_montgomery: c_int, d_out_xyz: *mut c_void) -> c_int;
    pub fn capgpu_msm_var_plan(n: usize, count: c_int, buf: *mut c_char, cap: usize) -> c_int;
    pub fn capgpu_g1_sum(points_xyz: *const u64, n: usize, out_xyz: *mut u64) -> c_int;
    // ---- one process per GPU: the RCCL exchange
    pub fn capgpu_comm_unique_id(id_out: *mut u8) -> c_int;
    pub fn capgpu_comm_init(rank: c_int, world: c_int, id: *const u8) -> c_int;
    pub fn capgpu_comm_init_loopback(world: c_int) -> c_int;
    pub fn capgpu_comm_loopback_set_rank(rank: c_int) -> c_int;
    pub fn capgpu_comm_destroy() -> c_int;
    pub fn capgpu_comm_info(rank_out: *mut c_int, world_out: *mut c_int) -> c_int;
    pub fn capgpu_msm_g1_sharded_dev(srs_handle: u64, offset: usize, d_scalars: *const c_void, scalar_stride: usize,
                                     n_local: usize, count: c_int, scalars_montgomery: c_int,
                                     d_out_xyz: *mut c_void) -> c_int;
    pub fn capgpu_msm_g1_sharded(srs_handle: u64, offset: usize, scalars: *const u64, n_local: usize,
                                 out_xyz: *mut u64) -> c_int;
    pub fn capgpu_plonk_shard_msm(on: c_int) -> c_int;
    // ---- NTT
    pub fn capgpu_ntt_fr(data: *mut u64, log_n: u32, dir: c_int, coset: c_int) -> c_int;
    pub fn capgpu_ntt_fr_batch(data: *const *mut u64, count: c_int, log_n: u32, dir: c_int, coset: c_int) -> c_int;
    pub fn capgpu_ntt_fr_dev(d_data: *mut c_void, stride_elems: usize, count: c_int, log_n: u32, dir: c_int,
                             coset: c_int) -> c_int;
    pub fn capgpu_ntt_plan(log_n: u32, count: c_int, out: *mut capgpu_ntt_plan_info) -> c_int;
    // ---- PLONK
    pub fn capgpu_plonk_preprocess(srs_handle: u64, n: usize, num_inputs: usize, selectors: *const u64,
                                   sigma_evals: *const u64, pk_handle_out: *mut u64,
                                   vk_out: *mut capgpu_verifying_key) -> c_int;
    pub fn capgpu_plonk_preprocess_ex(srs_handle: u64, n: usize, num_inputs: usize, selectors: *const u64,
                                      sigmas: *const u64, input_form: c_int, pk_handle_out: *mut u64,
                                      vk_out: *mut capgpu_verifying_key) -> c_int;
    pub fn capgpu_plonk_preprocess_vars(srs_handle: u64, n: usize, num_inputs: usize, selectors: *const u64,
                                        selector_form: c_int, wire_vars: *const u32, num_vars: usize,
                                        pk_handle_out: *mut u64, vk_out: *mut capgpu_verifying_key) -> c_int;
    pub fn capgpu_plonk_key_set_vars(pk_handle: u64, wire_vars: *const u32, num_vars: usize) -> c_int;
    pub fn capgpu_plonk_key_num_vars(pk_handle: u64, num_vars_out: *mut usize) -> c_int;
    pub fn capgpu_plonk_key_set_given(pk_handle: u64, given_vars: *const u32, num_given: usize,
                                      info_out: *mut capgpu_solver_info) -> c_int;
    pub fn capgpu_plonk_key_solver_info(pk_handle: u64, info_out: *mut capgpu_solver_info) -> c_int;
    pub fn capgpu_plonk_key_set_given_hints(pk_handle: u64, given_vars: *const u32, num_given: usize,
                                            hints: *const capgpu_hint, num_hints: usize, targets: *const u32,
                                            num_targets: usize, info_out: *mut capgpu_solver_info,
                                            hint_info_out: *mut capgpu_hint_info) -> c_int;
    pub fn capgpu_plonk_key_hint_info(pk_handle: u64, info_out: *mut capgpu_hint_info) -> c_int;
    pub fn capgpu_plonk_key_set_solver(pk_handle: u64, given_vars: *const u32, num_given: usize,
                                       hints: *const capgpu_hint, num_hints: usize, targets: *const u32,
                                       num_targets: usize, flags: u32, info_out: *mut capgpu_solver_info,
                                       hint_info_out: *mut capgpu_hint_info) -> c_int;
    pub fn capgpu_plonk_key_solver_rules_info(pk_handle: u64, info_out: *mut capgpu_solver_rules_info) -> c_int;
    pub fn capgpu_plonk_key_set_solve_form(pk_handle: u64, form: c_int, info_out: *mut capgpu_solve_form_info) -> c_int;
    pub fn capgpu_plonk_key_solve_form_info(pk_handle: u64, info_out: *mut capgpu_solve_form_info) -> c_int;
    pub fn capgpu_plonk_pub_inputs(pk_handle: u64, count: c_int, vars: *const u64, pub_out: *mut u64) -> c_int;
    pub fn capgpu_plonk_pub_inputs_dev(pk_handle: u64, count: c_int, d_vars: *const c_void, d_pub_out: *mut c_void) -> c_int;
    pub fn capgpu_plonk_solve_vars(pk_handle: u64, count: c_int, given: *const u64, vars_out: *mut u64,
                                   status_out: *mut capgpu_solve_status) -> c_int;
    pub fn capgpu_plonk_solve_vars_dev(pk_handle: u64, count: c_int, d_given: *const c_void, d_vars_out: *mut c_void,
                                       status_out: *mut capgpu_solve_status) -> c_int;
    pub fn capgpu_plonk_input_stats(witness_bytes_h2d_out: *mut u64, gather_launches_out: *mut u64) -> c_int;
    pub fn capgpu_plonk_free_key(pk_handle: u64) -> c_int;
    pub fn capgpu_plonk_key_info(pk_handle: u64, domain_size_out: *mut usize, num_inputs_out: *mut usize,
                                 srs_handle_out: *mut u64) -> c_int;
    pub fn capgpu_plonk_prove(pk_handle: u64, wires: *const u64, pub_inputs: *const u64, num_inputs: usize,
                              ext_msg: *const u8, ext_msg_len: usize, blinders: *const u64,
                              proof_out: *mut capgpu_proof) -> c_int;
    pub fn capgpu_plonk_set_coalescing(window_us: u32, max_batch: u32) -> c_int;
    pub fn capgpu_plonk_set_wire_commit(mode: c_int) -> c_int;
    pub fn capgpu_plonk_graph_stats(segments_captured_out: *mut u64, segments_replayed_out: *mut u64) -> c_int;
    pub fn capgpu_plonk_coalescing_stats(batches_out: *mut u64, proofs_out: *mut u64) -> c_int;
    pub fn capgpu_plonk_set_transcript(mode: c_int) -> c_int;
    pub fn capgpu_plonk_get_transcript(mode_out: *mut c_int) -> c_int;
    pub fn capgpu_plonk_sync_stats(prove_calls_out: *mut u64, stream_waits_out: *mut u64) -> c_int;
    pub fn capgpu_keccak256_batch_dev(data: *const u8, offsets: *const u64, count: c_int, digests_out: *mut u8) -> c_int;
    pub fn capgpu_plonk_prove_batch(pk_handle: u64, count: c_int, wires: *const u64, pub_inputs: *const u64,
                                    num_inputs: usize, ext_msg: *const u8, ext_msg_len: usize, blinders: *const u64,
                                    proofs_out: *mut capgpu_proof) -> c_int;
    pub fn capgpu_plonk_prove_multi(pk_handles: *const u64, count: c_int, wires: *const u64, pub_inputs: *const u64,
                                    num_inputs: usize, ext_msgs: *const *const u8, ext_msg_lens: *const usize,
                                    blinders: *const u64, proofs_out: *mut capgpu_proof) -> c_int;
    pub fn capgpu_plonk_prove_multi_dev(pk_handles: *const u64, count: c_int, d_wires: *const c_void,
                                        pub_inputs: *const u64, num_inputs: usize, ext_msgs: *const *const u8,
                                        ext_msg_lens: *const usize, blinders: *const u64,
                                        proofs_out: *mut capgpu_proof) -> c_int;
    pub fn capgpu_plonk_prove_batch_dev(pk_handle: u64, count: c_int, d_wires: *const c_void, pub_inputs: *const u64,
                                        num_inputs: usize, ext_msg: *const u8, ext_msg_len: usize,
                                        blinders: *const u64, proofs_out: *mut capgpu_proof) -> c_int;
    pub fn capgpu_plonk_prove_ex(pk_handle: u64, wires: *const u64, pub_inputs: *const u64, num_inputs: usize,
                                 ext_msg: *const u8, ext_msg_len: usize, blinders: *const u64, input_form: c_int,
                                 proof_out: *mut capgpu_proof) -> c_int;
    pub fn capgpu_plonk_prove_batch_ex(pk_handle: u64, count: c_int, wires: *const u64, pub_inputs: *const u64,
                                       num_inputs: usize, ext_msg: *const u8, ext_msg_len: usize,
                                       blinders: *const u64, input_form: c_int, proofs_out: *mut capgpu_proof) -> c_int;
    pub fn capgpu_plonk_prove_multi_ex(pk_handles: *const u64, count: c_int, wires: *const u64,
                                       pub_inputs: *const u64, num_inputs: usize, ext_msgs: *const *const u8,
                                       ext_msg_lens: *const usize, blinders: *const u64, input_form: c_int,
                                       proofs_out: *mut capgpu_proof) -> c_int;
    pub fn capgpu_plonk_prove_multi_dev_ex(pk_handles: *const u64, count: c_int, d_wires: *const c_void,
                                           pub_inputs: *const u64, num_inputs: usize, ext_msgs: *const *const u8,
                                           ext_msg_lens: *const usize, blinders: *const u64, input_form: c_int,
                                           proofs_out: *mut capgpu_proof) -> c_int;
    pub fn capgpu_plonk_prove_batch_dev_ex(pk_handle: u64, count: c_int, d_wires: *const c_void,
                                           pub_inputs: *const u64, num_inputs: usize, ext_msg: *const u8,
                                           ext_msg_len: usize, blinders: *const u64, input_form: c_int,
                                           proofs_out: *mut capgpu_proof) -> c_int;
    // ---- witness check (Circuit::check_circuit_satisfiability as the reference's prove() calls it)
    pub fn capgpu_plonk_check_witness(pk_handle: u64, wires: *const u64, pub_inputs: *const u64, num_inputs: usize,
                                      input_form: c_int, fault_out: *mut capgpu_witness_fault) -> c_int;
    pub fn capgpu_plonk_check_witness_batch(pk_handle: u64, count: c_int, wires: *const u64, pub_inputs: *const u64,
                                            num_inputs: usize, input_form: c_int,
                                            faults_out: *mut capgpu_witness_fault) -> c_int;
    pub fn capgpu_plonk_check_witness_batch_dev(pk_handle: u64, count: c_int, d_wires: *const c_void,
                                                pub_inputs: *const u64, num_inputs: usize, input_form: c_int,
                                                faults_out: *mut capgpu_witness_fault) -> c_int;
    pub fn capgpu_plonk_check_witness_multi(pk_handles: *const u64, count: c_int, wires: *const u64,
                                            pub_inputs: *const u64, num_inputs: usize, input_form: c_int,
                                            faults_out: *mut capgpu_witness_fault) -> c_int;
    pub fn capgpu_plonk_set_precheck(on: c_int) -> c_int;

    pub fn capgpu_plonk_prove_batch_async(pk_handle: u64, count: c_int, wires: *const u64, pub_inputs: *const u64,
                                          num_inputs: usize, ext_msg: *const u8, ext_msg_len: usize,
                                          blinders: *const u64, input_form: c_int, proofs_out: *mut capgpu_proof,
                                          ticket_out: *mut u64) -> c_int;
    pub fn capgpu_plonk_prove_multi_async(pk_handles: *const u64, count: c_int, wires: *const u64,
                                          pub_inputs: *const u64, num_inputs: usize, ext_msgs: *const *const u8,
                                          ext_msg_lens: *const usize, blinders: *const u64, input_form: c_int,
                                          proofs_out: *mut capgpu_proof, ticket_out: *mut u64) -> c_int;
    pub fn capgpu_wait(ticket: u64, timeout_ms: u32, done_out: *mut c_int) -> c_int;
    // ---- per-proof outcomes: a batch is proved past its unsatisfied witnesses
    pub fn capgpu_plonk_prove_each(pk_handles: *const u64, count: c_int, wires: *const u64, pub_inputs: *const u64,
                                   num_inputs: usize, ext_msgs: *const *const u8, ext_msg_lens: *const usize,
                                   blinders: *const u64, input_form: c_int, proofs_out: *mut capgpu_proof,
                                   outcomes_out: *mut capgpu_prove_outcome) -> c_int;
    pub fn capgpu_plonk_prove_each_dev(pk_handles: *const u64, count: c_int, d_wires: *const c_void,
                                       pub_inputs: *const u64, num_inputs: usize, ext_msgs: *const *const u8,
                                       ext_msg_lens: *const usize, blinders: *const u64, input_form: c_int,
                                       proofs_out: *mut capgpu_proof, outcomes_out: *mut capgpu_prove_outcome) -> c_int;
    pub fn capgpu_plonk_prove_each_async(pk_handles: *const u64, count: c_int, wires: *const u64,
                                         pub_inputs: *const u64, num_inputs: usize, ext_msgs: *const *const u8,
                                         ext_msg_lens: *const usize, blinders: *const u64, input_form: c_int,
                                         proofs_out: *mut capgpu_proof, outcomes_out: *mut capgpu_prove_outcome,
                                         ticket_out: *mut u64) -> c_int;
    pub fn capgpu_prove_outcome_text(outcome: *const capgpu_prove_outcome, buf: *mut c_char, cap: usize) -> c_int;
    // ---- a Vec of notes whose keys have several domain sizes (or SRS) in one call
    pub fn capgpu_plonk_prove_notes(pk_handles: *const u64, count: c_int, wires: *const *const u64, pub_inputs: *const u64,
                                    num_inputs: usize, ext_msgs: *const *const u8, ext_msg_lens: *const usize,
                                    blinders: *const u64, input_form: c_int, proofs_out: *mut capgpu_proof,
                                    outcomes_out: *mut capgpu_prove_outcome) -> c_int;
    pub fn capgpu_plonk_prove_notes_dev(pk_handles: *const u64, count: c_int, d_wires: *const c_void,
                                        wire_offsets: *const u64, pub_inputs: *const u64, num_inputs: usize,
                                        ext_msgs: *const *const u8, ext_msg_lens: *const usize, blinders: *const u64,
                                        input_form: c_int, proofs_out: *mut capgpu_proof,
                                        outcomes_out: *mut capgpu_prove_outcome) -> c_int;
    pub fn capgpu_plonk_prove_notes_async(pk_handles: *const u64, count: c_int, wires: *const *const u64,
                                          pub_inputs: *const u64, num_inputs: usize, ext_msgs: *const *const u8,
                                          ext_msg_lens: *const usize, blinders: *const u64, input_form: c_int,
                                          proofs_out: *mut capgpu_proof, outcomes_out: *mut capgpu_prove_outcome,
                                          ticket_out: *mut u64) -> c_int;
    pub fn capgpu_plonk_notes_plan(pk_handles: *const u64, count: c_int, groups_out: *mut capgpu_notes_group, cap: usize,
                                   num_groups_out: *mut usize, group_of_out: *mut u32) -> c_int;
    pub fn capgpu_plonk_reserve_notes(pk_handles: *const u64, count: c_int, input_form: c_int, slot: c_int) -> c_int;
    pub fn capgpu_plonk_notes_stats(out: *mut capgpu_notes_stats) -> c_int;
    // ---- batch compaction of the outcome calls: witnesses the check refused leave the batch before round 1
    pub fn capgpu_plonk_set_compaction(on: c_int) -> c_int;
    pub fn capgpu_plonk_get_compaction(on_out: *mut c_int) -> c_int;
    pub fn capgpu_plonk_compaction_stats(calls_out: *mut u64, proofs_dropped_out: *mut u64,
                                         rows_moved_out: *mut u64) -> c_int;
    pub fn capgpu_async_stats(submitted_out: *mut u64, completed_out: *mut u64, max_running_out: *mut u32) -> c_int;
    pub fn capgpu_plonk_reserve(pk_handle: u64, count: c_int, input_form: c_int, slot: c_int) -> c_int;
    // ---- proving from the values a circuit is given: the solver and the variable-form outcome call in one
    pub fn capgpu_plonk_set_solve_pack(w: c_int) -> c_int;
    pub fn capgpu_plonk_get_solve_pack(w_out: *mut c_int) -> c_int;
    pub fn capgpu_plonk_solve_stats(launches_out: *mut u64, witnesses_out: *mut u64,
                                    packed_launches_out: *mut u64) -> c_int;
    // ---- Fr inversion: the form the solver's launches and the batch calls run (CAPGPU_INVERSE_*), the batch inverse
    pub fn capgpu_fr_set_inverse_form(form: c_int) -> c_int;
    pub fn capgpu_fr_get_inverse_form(form_out: *mut c_int) -> c_int;
    pub fn capgpu_fr_inverse_batch(h_in: *const c_void, h_out: *mut c_void, count: usize) -> c_int;
    pub fn capgpu_fr_inverse_batch_dev(d_in: *const c_void, d_out: *mut c_void, count: usize) -> c_int;
    pub fn capgpu_fr_inverse_stats(fermat_launches_out: *mut u64, gcd_launches_out: *mut u64) -> c_int;
    pub fn capgpu_plonk_prove_given(pk_handles: *const u64, count: c_int, given: *const u64, pub_inputs: *const u64,
                                    num_inputs: usize, ext_msgs: *const *const u8, ext_msg_lens: *const usize,
                                    blinders: *const u64, proofs_out: *mut capgpu_proof,
                                    outcomes_out: *mut capgpu_prove_outcome,
                                    solved_out: *mut capgpu_solve_status) -> c_int;
    pub fn capgpu_plonk_prove_given_dev(pk_handles: *const u64, count: c_int, d_given: *const c_void,
                                        pub_inputs: *const u64, num_inputs: usize, ext_msgs: *const *const u8,
                                        ext_msg_lens: *const usize, blinders: *const u64,
                                        proofs_out: *mut capgpu_proof, outcomes_out: *mut capgpu_prove_outcome,
                                        solved_out: *mut capgpu_solve_status) -> c_int;
    pub fn capgpu_plonk_prove_given_async(pk_handles: *const u64, count: c_int, given: *const u64,
                                          pub_inputs: *const u64, num_inputs: usize, ext_msgs: *const *const u8,
                                          ext_msg_lens: *const usize, blinders: *const u64,
                                          proofs_out: *mut capgpu_proof, outcomes_out: *mut capgpu_prove_outcome,
                                          solved_out: *mut capgpu_solve_status, ticket_out: *mut u64) -> c_int;
    pub fn capgpu_plonk_prove_given_io(pk_handles: *const u64, count: c_int, given: *const u64, num_inputs: usize,
                                       ext_msgs: *const *const u8, ext_msg_lens: *const usize, blinders: *const u64,
                                       pub_inputs_out: *mut u64, proofs_out: *mut capgpu_proof,
                                       outcomes_out: *mut capgpu_prove_outcome,
                                       solved_out: *mut capgpu_solve_status) -> c_int;
    pub fn capgpu_plonk_prove_given_io_dev(pk_handles: *const u64, count: c_int, d_given: *const c_void, num_inputs: usize,
                                           ext_msgs: *const *const u8, ext_msg_lens: *const usize, blinders: *const u64,
                                           pub_inputs_out: *mut u64, proofs_out: *mut capgpu_proof,
                                           outcomes_out: *mut capgpu_prove_outcome,
                                           solved_out: *mut capgpu_solve_status) -> c_int;
    pub fn capgpu_plonk_prove_given_io_async(pk_handles: *const u64, count: c_int, given: *const u64, num_inputs: usize,
                                             ext_msgs: *const *const u8, ext_msg_lens: *const usize,
                                             blinders: *const u64, pub_inputs_out: *mut u64,
                                             proofs_out: *mut capgpu_proof, outcomes_out: *mut capgpu_prove_outcome,
                                             solved_out: *mut capgpu_solve_status, ticket_out: *mut u64) -> c_int;
    pub fn capgpu_plonk_reserve_given(pk_handle: u64, count: c_int, slot: c_int) -> c_int;
    pub fn capgpu_plonk_prove_given_one(pk_handle: u64, given: *const u64, num_given: usize, pub_inputs: *const u64,
                                        num_inputs: usize, ext_msg: *const u8, ext_msg_len: usize, blinders: *const u64,
                                        proof_out: *mut capgpu_proof, outcome_out: *mut capgpu_prove_outcome,
                                        solved_out: *mut capgpu_solve_status) -> c_int;
    pub fn capgpu_plonk_prove_given_io_one(pk_handle: u64, given: *const u64, num_given: usize, num_inputs: usize,
                                           ext_msg: *const u8, ext_msg_len: usize, blinders: *const u64,
                                           pub_inputs_out: *mut u64, proof_out: *mut capgpu_proof,
                                           outcome_out: *mut capgpu_prove_outcome,
                                           solved_out: *mut capgpu_solve_status) -> c_int;
    // ---- verification (host only)
    pub fn capgpu_g2_generator(out: *mut u64) -> c_int;
    pub fn capgpu_g2_mul(q: *const u64, scalar: *const u64, out: *mut u64) -> c_int;
    pub fn capgpu_pairing_check(g1_points: *const u64, g2_points: *const u64, n: usize, ok_out: *mut c_int) -> c_int;
    pub fn capgpu_plonk_verify(vk: *const capgpu_verifying_key, g2_h: *const u64, g2_beta_h: *const u64,
                               pub_inputs: *const u64, num_inputs: usize, proof: *const capgpu_proof,
                               ext_msg: *const u8, ext_msg_len: usize, ok_out: *mut c_int) -> c_int;
    pub fn capgpu_plonk_batch_verify(vks: *const *const capgpu_verifying_key, g2_h: *const u64, g2_beta_h: *const u64,
                                     pub_inputs: *const *const u64, num_inputs: *const usize,
                                     proofs: *const *const capgpu_proof, ext_msgs: *const *const u8,
                                     ext_msg_lens: *const usize, count: usize, ok_out: *mut c_int) -> c_int;
    pub fn capgpu_plonk_batch_verify_dev(vks: *const *const capgpu_verifying_key, g2_h: *const u64,
                                         g2_beta_h: *const u64, pub_inputs: *const *const u64,
                                         num_inputs: *const usize, proofs: *const *const capgpu_proof,
                                         ext_msgs: *const *const u8, ext_msg_lens: *const usize, count: usize,
                                         ok_out: *mut c_int) -> c_int;
    // ---- per-proof verification on the device
    pub fn capgpu_pairing_check_pairs_dev(p: *const u64, r: *const u64, count: usize, q1: *const u64, q2: *const u64,
                                          ok_out: *mut c_int) -> c_int;
    pub fn capgpu_plonk_verify_each_dev(vks: *const *const capgpu_verifying_key, g2_h: *const u64,
                                        g2_beta_h: *const u64, pub_inputs: *const *const u64,
                                        num_inputs: *const usize, proofs: *const *const capgpu_proof,
                                        ext_msgs: *const *const u8, ext_msg_lens: *const usize, count: usize,
                                        ok_out: *mut c_int) -> c_int;
    // ---- the pairing check's two forms (CAPGPU_PAIRING_LANE / CAPGPU_PAIRING_WAVE)
    pub fn capgpu_pairing_set_form(form: c_int) -> c_int;
    pub fn capgpu_pairing_get_form(form_out: *mut c_int) -> c_int;
    pub fn capgpu_pairing_stats(lane_checks_out: *mut u64, wave_checks_out: *mut u64) -> c_int;
    pub fn capgpu_plonk_verify_dev(vk: *const capgpu_verifying_key, g2_h: *const u64, g2_beta_h: *const u64,
                                   pub_inputs: *const u64, num_inputs: usize, ext_msg: *const u8, ext_msg_len: usize,
                                   proof: *const capgpu_proof, ok_out: *mut c_int) -> c_int;
    pub fn capgpu_plonk_vk_upload(vk: *const capgpu_verifying_key, vk_handle_out: *mut u64) -> c_int;
    pub fn capgpu_plonk_vk_release(vk_handle: u64) -> c_int;
    pub fn capgpu_plonk_verify_block_dev(vk_handles: *const u64, g2_h: *const u64, g2_beta_h: *const u64,
                                         pub_inputs: *const u64, num_inputs: usize, proofs: *const capgpu_proof,
                                         ext_msgs: *const *const u8, ext_msg_lens: *const usize, count: usize,
                                         block_ok_out: *mut c_int, each_ok_out: *mut c_int) -> c_int;
    pub fn capgpu_plonk_verify_block_resident(vk_handles: *const u64, g2_h: *const u64, g2_beta_h: *const u64,
                                              d_pub_inputs: *const c_void, num_inputs: usize, d_proofs: *const c_void,
                                              ext_msgs: *const *const u8, ext_msg_lens: *const usize, count: usize,
                                              block_ok_out: *mut c_int, each_ok_out: *mut c_int) -> c_int;
    pub fn capgpu_verify_sync_stats(block_calls_out: *mut u64, stream_waits_out: *mut u64) -> c_int;
    pub fn capgpu_proof_serialize(proof: *const capgpu_proof, out: *mut u8, cap: usize, len_out: *mut usize) -> c_int;
    pub fn capgpu_proof_deserialize(bytes: *const u8, len: usize, proof_out: *mut capgpu_proof,
                                    consumed_out: *mut usize) -> c_int;
    pub fn capgpu_proof_decode_batch(bytes: *const u8, stride: usize, count: usize, proofs_out: *mut capgpu_proof,
                                     status_out: *mut c_int) -> c_int;
    pub fn capgpu_proof_decode_batch_dev(d_bytes: *const c_void, stride: usize, count: usize, d_proofs_out: *mut c_void,
                                         d_status_out: *mut c_int) -> c_int;
    pub fn capgpu_proof_encode_batch(proofs: *const capgpu_proof, count: usize, bytes_out: *mut u8, stride: usize) -> c_int;
    pub fn capgpu_proof_encode_batch_dev(d_proofs: *const c_void, count: usize, d_bytes_out: *mut c_void,
                                         stride: usize) -> c_int;
    pub fn capgpu_plonk_verify_block_bytes(vk_handles: *const u64, g2_h: *const u64, g2_beta_h: *const u64,
                                           pub_inputs: *const u64, num_inputs: usize, proof_bytes: *const u8, stride: usize,
                                           ext_msgs: *const *const u8, ext_msg_lens: *const usize, count: usize,
                                           block_ok_out: *mut c_int, each_ok_out: *mut c_int,
                                           decode_status_out: *mut c_int) -> c_int;
    pub fn capgpu_plonk_verify_block_bytes_resident(vk_handles: *const u64, g2_h: *const u64, g2_beta_h: *const u64,
                                                    d_pub_inputs: *const c_void, num_inputs: usize,
                                                    d_proof_bytes: *const c_void, stride: usize, ext_msgs: *const *const u8,
                                                    ext_msg_lens: *const usize, count: usize, block_ok_out: *mut c_int,
                                                    each_ok_out: *mut c_int, decode_status_out: *mut c_int) -> c_int;
    // ---- on-disk parameter formats
    pub fn capgpu_g1_decompress(input: *const u8, n: usize, out_xy: *mut u64) -> c_int;
    pub fn capgpu_g1_compress(xy: *const u64, n: usize, out: *mut u8) -> c_int;
    pub fn capgpu_srs_deserialize(bytes: *const u8, len: usize, max_degree: usize, handle_out: *mut u64,
                                  h_out: *mut u64, beta_h_out: *mut u64, consumed_out: *mut usize) -> c_int;
    pub fn capgpu_srs_serialize(handle: u64, h: *const u64, beta_h: *const u64, out: *mut u8, cap: usize,
                                len_out: *mut usize) -> c_int;
    pub fn capgpu_plonk_vk_serialize(vk: *const capgpu_verifying_key, g: *const u64, gamma_g: *const u64,
                                     h: *const u64, beta_h: *const u64, out: *mut u8, cap: usize,
                                     len_out: *mut usize) -> c_int;
    pub fn capgpu_plonk_vk_deserialize(bytes: *const u8, len: usize, vk_out: *mut capgpu_verifying_key,
                                       g_out: *mut u64, gamma_g_out: *mut u64, h_out: *mut u64, beta_h_out: *mut u64,
                                       consumed_out: *mut usize) -> c_int;
    pub fn capgpu_plonk_key_serialize(pk_handle: u64, gamma_g: *const u64, h: *const u64, beta_h: *const u64,
                                      out: *mut u8, cap: usize, len_out: *mut usize) -> c_int;
    pub fn capgpu_plonk_key_deserialize(bytes: *const u8, len: usize, srs_handle_out: *mut u64,
                                        pk_handle_out: *mut u64, vk_out: *mut capgpu_verifying_key, h_out: *mut u64,
                                        beta_h_out: *mut u64, consumed_out: *mut usize) -> c_int;
    // ---- parameter audit
    pub fn capgpu_srs_check(srs_handle: u64, g2_h: *const u64, g2_beta_h: *const u64, seed: *const u8, flags: u32,
                            out: *mut capgpu_srs_report) -> c_int;
    pub fn capgpu_plonk_key_check(pk_handle: u64, vk: *const capgpu_verifying_key, out: *mut capgpu_key_report) -> c_int;
    // ---- instrumentation
    pub fn capgpu_ubench_mad_rate(lane_ops_per_s_out: *mut f64) -> c_int;
    pub fn capgpu_ubench_issue_rates(rates_out: *mut f64, count: c_int) -> c_int;
    pub fn capgpu_profile_enable(on: c_int) -> c_int;
    pub fn capgpu_profile_reset() -> c_int;
    pub fn capgpu_profile_get(name: *const c_char, total_ms_out: *mut f64, launches_out: *mut u64) -> c_int;
    pub fn capgpu_profile_dump(buf: *mut c_char, cap: usize) -> c_int;
}

// ---------------------------------------------------------------------------------------------------------------
// Safe layer.  Error = (code, thread-local message); the caller maps it to `PlonkError`, which the reference's
// prove() already maps to `TxnApiError::FailedSnark(String)` (src/proof/transfer.rs:187), and
// `CAPGPU_ERR_SERIALIZATION` to `TxnApiError::DeserializationError` (src/errors.rs:81-90).
// ---------------------------------------------------------------------------------------------------------------
#[derive(Debug, Clone)]
pub struct Error {
    pub code: i32,
    pub message: String,
}
impl std::fmt::Display for Error {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        write!(f, "capgpu error {}: {}", self.code, self.message)
    }
}
impl std::error::Error for Error {}
pub type Result<T> = std::result::Result<T, Error>;

pub fn check(rc: c_int) -> Result<()> {
    if rc == CAPGPU_OK {
        return Ok(());
    }
    let message = unsafe { std::ffi::CStr::from_ptr(capgpu_last_error()) }.to_string_lossy().into_owned();
    Err(Error { code: rc, message })
}

/// Binds the process to the listed HIP devices (idempotent).  With more than one, the library deals host-buffer
/// batches and coalesced `prove` calls over them by itself: the rayon loop of
/// `TxnsParams::generate_txns` (src/utils/params_builder.rs:194-226) needs no change to use every GPU of the node.
pub fn init(devices: &[i32]) -> Result<()> {
    check(unsafe { capgpu_init(if devices.is_empty() { std::ptr::null() } else { devices.as_ptr() }, devices.len() as c_int) })
}

/// Gather concurrent single-proof calls into device batches (what a rayon `par_iter` over notes produces).
pub fn set_coalescing(window_us: u32, max_batch: u32) -> Result<()> {
    check(unsafe { capgpu_plonk_set_coalescing(window_us, max_batch) })
}

/// How the wire commitments are computed: `true` (the default) from the witness VALUES on the Lagrange-form key - round 1's
/// time then depends on the witness's sparsity -, `false` from coefficients, as jf-plonk does (witness-independent work;
/// the mode for deployments where an adversary can time proofs: include/capgpu.h, "TIMING AND THE SECRET WITNESS").
pub fn set_wire_commit_from_evals(on: bool) -> Result<()> {
    check(unsafe { capgpu_plonk_set_wire_commit(if on { 1 } else { 0 }) })
}

/// `form` of `capgpu_pairing_set_form`: one pairing check per lane (the default), or one per group of six lanes.
pub const CAPGPU_PAIRING_LANE: c_int = 0;
pub const CAPGPU_PAIRING_WAVE: c_int = 1;

pub const CAPGPU_INVERSE_FERMAT: c_int = 0;
pub const CAPGPU_INVERSE_GCD: c_int = 1;
pub const CAPGPU_TRANSCRIPT_HOST: c_int = 0;
pub const CAPGPU_TRANSCRIPT_DEVICE: c_int = 1;

/// Where the Fiat-Shamir transcript of the next prove calls runs: `true` on the device - the five rounds are enqueued
/// without a host wait and the call synchronises once -, `false` (the default) on the host.  Same proof bytes.
pub fn set_transcript_on_device(on: bool) -> Result<()> {
    check(unsafe { capgpu_plonk_set_transcript(if on { CAPGPU_TRANSCRIPT_DEVICE } else { CAPGPU_TRANSCRIPT_HOST }) })
}

/// (device batches proved, host waits on the proving stream inside them) since process start.
pub fn sync_stats() -> Result<(u64, u64)> {
    let (mut calls, mut waits) = (0u64, 0u64);
    check(unsafe { capgpu_plonk_sync_stats(&mut calls, &mut waits) })?;
    Ok((calls, waits))
}

/// Releases the workspace of every idle device context (scratch, pinned result areas, captured launch graphs): tables -
/// SRS, proving keys, NTT domains - stay.  Returns the device bytes given back.  A process that shares the GPU calls this
/// when it goes idle; the next proof allocates again.
pub fn trim() -> Result<u64> {
    let mut released = 0u64;
    let mut busy: c_int = 0;
    check(unsafe { capgpu_trim(&mut released, &mut busy) })?;
    Ok(released)
}

/// Caps the workspace the library holds per device (0 = no cap).  A `prove` that would grow past it fails with
/// `CAPGPU_ERR_OOM` (after trimming the device's idle contexts): prove in smaller batches, or raise the cap.
pub fn set_memory_limit(scratch_bytes_per_device: u64) -> Result<()> {
    check(unsafe { capgpu_set_memory_limit(scratch_bytes_per_device) })
}

/// (growths of scratch buffers and pinned areas since `init`, bytes of new capacity, milliseconds spent growing): read
/// around a timed section - a non-zero difference says an allocation landed inside it (`ProvingKey::reserve` avoids it).
pub fn scratch_stats() -> Result<(u64, u64, f64)> {
    let (mut events, mut bytes, mut ms) = (0u64, 0u64, 0f64);
    check(unsafe { capgpu_scratch_stats(&mut events, &mut bytes, &mut ms) })?;
    Ok((events, bytes, ms))
}

/// (tickets accepted, tickets finished, most running at once on one device) since `init`.
pub fn async_stats() -> Result<(u64, u64, u32)> {
    let (mut submitted, mut completed, mut max_running) = (0u64, 0u64, 0u32);
    check(unsafe { capgpu_async_stats(&mut submitted, &mut completed, &mut max_running) })?;
    Ok((submitted, completed, max_running))
}

/// A device-resident commit key (`UniversalSrs::powers_of_g` / `CommitKey::powers_of_g`).
pub struct Srs {
    handle: u64,
}
impl Srs {
    /// `bases`: arkworks `GroupAffine` values as they sit in memory.  `stride` = `size_of::<G1Affine>()` (72 with the
    /// `infinity` flag byte at offset 64; `GroupAffine` is `repr(Rust)` - assert the offsets in the caller's tests) or
    /// 64 for packed (x, y) pairs.
    ///
    /// # Safety
    /// `bases` must point to `n * stride` readable bytes.
    pub unsafe fn upload_raw(bases: *const u8, n: usize, stride: usize) -> Result<Srs> {
        let mut handle = 0u64;
        check(capgpu_srs_upload(bases as *const c_void, n, stride, 1, &mut handle))?;
        Ok(Srs { handle })
    }
    /// The bytes of an ark-serialized `UniversalSrs` (`load_srs`, src/proof/mod.rs:106; `load_universal_parameter`,
    /// src/parameters.rs:97-109).  Returns the SRS and the open key's (h, beta_h).
    pub fn deserialize(bytes: &[u8], max_degree: usize) -> Result<(Srs, [u64; 16], [u64; 16])> {
        let (mut handle, mut used) = (0u64, 0usize);
        let (mut h, mut beta_h) = ([0u64; 16], [0u64; 16]);
        check(unsafe {
            capgpu_srs_deserialize(bytes.as_ptr(), bytes.len(), max_degree, &mut handle, h.as_mut_ptr(),
                                   beta_h.as_mut_ptr(), &mut used)
        })?;
        Ok((Srs { handle }, h, beta_h))
    }
    /// Is this SRS `[tau^i] g` for the tau of the open key `(h, beta_h)`?  What `load_srs` guards with a SHA-256 over the
    /// file (src/proof/mod.rs:95-102), asked of the points themselves: once per loaded file, not per proof.  `seed`:
    /// `None` draws the fold's weights from the OS (the sound choice), `Some` makes the report reproducible; `locate`
    /// finds the first bad link of an inconsistent SRS.  `Ok` whenever the check ran: the verdict is in the report.
    pub fn check(&self, h: &[u64; 16], beta_h: &[u64; 16], seed: Option<&[u8; 32]>, locate: bool) -> Result<capgpu_srs_report> {
        let mut rep = capgpu_srs_report::default();
        check(unsafe {
            capgpu_srs_check(self.handle, h.as_ptr(), beta_h.as_ptr(), seed.map_or(std::ptr::null(), |s| s.as_ptr()),
                             if locate { CAPGPU_SRS_CHECK_LOCATE } else { 0 }, &mut rep)
        })?;
        Ok(rep)
    }
    pub fn handle(&self) -> u64 {
        self.handle
    }
    pub fn len(&self) -> Result<usize> {
        let mut n = 0usize;
        check(unsafe { capgpu_srs_size(self.handle, &mut n) })?;
        Ok(n)
    }
    /// `VariableBaseMSM::multi_scalar_mul(&bases[offset..offset + scalars.len()], scalars)`: `scalars` are canonical
    /// integers (`into_repr()`), 4 words each; the result is (X, Y, Z) of a `GroupProjective`, Montgomery words.
    pub fn msm(&self, offset: usize, scalars: &[[u64; 4]]) -> Result<[u64; 12]> {
        let mut out = [0u64; 12];
        check(unsafe { capgpu_msm_g1(self.handle, offset, scalars.as_ptr() as *const u64, scalars.len(), out.as_mut_ptr()) })?;
        Ok(out)
    }
}
impl Drop for Srs {
    fn drop(&mut self) {
        unsafe { capgpu_srs_free(self.handle) };
    }
}

/// `VariableBaseMSM::multi_scalar_mul(bases, scalars)` for bases that were never uploaded: packed (x, y) pairs in
/// arkworks' Montgomery words ((0, 0) = infinity), canonical scalars (`into_repr()`); the result is (X, Y, Z) of a
/// `GroupProjective`.  Nothing stays on the device.  Bases that serve many MSMs belong in an [`Srs`] instead.
pub fn multi_scalar_mul(bases: &[[u64; 8]], scalars: &[[u64; 4]]) -> Result<[u64; 12]> {
    let n = bases.len().min(scalars.len()); // (as ark-ec: the shorter of the two)
    let mut out = [0u64; 12];
    check(unsafe {
        capgpu_msm_g1_var(bases.as_ptr() as *const c_void, 64, 1, scalars.as_ptr() as *const u64, n, out.as_mut_ptr())
    })?;
    Ok(out)
}

/// `Radix2EvaluationDomain::{fft, ifft, coset_fft, coset_ifft}_in_place` on a `Vec<Fr>` viewed as words.
pub fn ntt_in_place(data: &mut [[u64; 4]], inverse: bool, coset: bool) -> Result<()> {
    assert!(data.len().is_power_of_two());
    check(unsafe {
        capgpu_ntt_fr(data.as_mut_ptr() as *mut u64, data.len().trailing_zeros(), inverse as c_int, coset as c_int)
    })
}

/// A device-resident proving key (`jf_plonk::proof_system::structs::ProvingKey`).
pub struct ProvingKey {
    handle: u64,
    pub vk: capgpu_verifying_key,
    pub domain_size: usize,
    pub num_inputs: usize,
}
impl ProvingKey {
    /// `PlonkKzgSnark::preprocess(srs, circuit)` from the circuit's tables of VALUES on the domain
    /// (`CAPGPU_INPUT_EVALS`): `selectors` = 13 columns (q_lc x4, q_mul x2, q_hash x4, q_o, q_c, q_ecc), `sigma` = the 5
    /// extended-permutation columns, n values each, column-major, Montgomery words.  This name has meant EVALUATIONS
    /// since round 1 and keeps meaning it: a caller holding jf-relation's polynomials uses `preprocess_coeffs` - the two
    /// forms cannot be told apart from the data, so the form is in the function name, not in a default.
    pub fn preprocess(srs: &Srs, n: usize, num_inputs: usize, selectors: &[[u64; 4]], sigma: &[[u64; 4]]) -> Result<ProvingKey> {
        Self::preprocess_form(srs, n, num_inputs, selectors, sigma, CAPGPU_INPUT_EVALS)
    }
    /// The same from POLYNOMIALS in coefficient form (`CAPGPU_INPUT_COEFFS`):
    /// `arkworks::poly_columns(&circuit.compute_selector_polynomials()?, n)` and
    /// `..compute_extended_permutation_polynomials()`, passed through as jf-relation computed them (no transform on the
    /// CPU; the device evaluates sigma where round 2 needs its values).  Same key bytes as `preprocess` on the values.
    pub fn preprocess_coeffs(srs: &Srs, n: usize, num_inputs: usize, selector_polys: &[[u64; 4]], sigma_polys: &[[u64; 4]]) -> Result<ProvingKey> {
        Self::preprocess_form(srs, n, num_inputs, selector_polys, sigma_polys, CAPGPU_INPUT_COEFFS)
    }
    /// Either form, stated explicitly (`CAPGPU_INPUT_EVALS` / `CAPGPU_INPUT_COEFFS`).
    pub fn preprocess_form(srs: &Srs, n: usize, num_inputs: usize, selectors: &[[u64; 4]], sigma: &[[u64; 4]],
                           input_form: c_int) -> Result<ProvingKey> {
        assert_eq!(selectors.len(), NUM_SELECTORS * n);
        assert_eq!(sigma.len(), NUM_WIRE_TYPES * n);
        let mut handle = 0u64;
        let mut vk: capgpu_verifying_key = unsafe { std::mem::zeroed() };
        check(unsafe {
            capgpu_plonk_preprocess_ex(srs.handle, n, num_inputs, selectors.as_ptr() as *const u64,
                                       sigma.as_ptr() as *const u64, input_form, &mut handle, &mut vk)
        })?;
        Ok(ProvingKey { handle, vk, domain_size: n, num_inputs })
    }
    /// `PlonkKzgSnark::preprocess` from what a jf-relation `PlonkCircuit` holds about its copy constraints: the wire ->
    /// variable table, `circuit.wire_variables[..5]` flattened column-major (5 columns of n ids below `num_vars` =
    /// `circuit.num_vars()`).  The permutation is built on the device; the key bytes are those of `preprocess` on the
    /// permutation's values.  The key keeps the table: it is the one that `prove_vars` works with.  `selectors` in
    /// `selector_form` (`CAPGPU_INPUT_EVALS` / `CAPGPU_INPUT_COEFFS`).
    pub fn preprocess_vars(srs: &Srs, n: usize, num_inputs: usize, selectors: &[[u64; 4]], selector_form: c_int,
                           wire_vars: &[u32], num_vars: usize) -> Result<ProvingKey> {
        assert_eq!(selectors.len(), NUM_SELECTORS * n);
        assert_eq!(wire_vars.len(), NUM_WIRE_TYPES * n);
        let mut handle = 0u64;
        let mut vk: capgpu_verifying_key = unsafe { std::mem::zeroed() };
        check(unsafe {
            capgpu_plonk_preprocess_vars(srs.handle, n, num_inputs, selectors.as_ptr() as *const u64, selector_form,
                                         wire_vars.as_ptr(), num_vars, &mut handle, &mut vk)
        })?;
        Ok(ProvingKey { handle, vk, domain_size: n, num_inputs })
    }
    /// Does this key commit to `vk` (`None`: the key's own - the one a deserialised blob carried, which `load_data`,
    /// src/parameters.rs:560-577, takes on faith)?  `Ok` whenever the check ran: the verdict is in the report.
    pub fn check(&self, vk: Option<&capgpu_verifying_key>) -> Result<capgpu_key_report> {
        let mut rep = capgpu_key_report::default();
        check(unsafe {
            capgpu_plonk_key_check(self.handle, vk.map_or(std::ptr::null(), |v| v as *const capgpu_verifying_key), &mut rep)
        })?;
        Ok(rep)
    }
    /// Attaches the table to a key made another way (`preprocess`, a deserialised blob); refused when the permutation
    /// it implies is not the key's.
    pub fn set_vars(&self, wire_vars: &[u32], num_vars: usize) -> Result<()> {
        assert_eq!(wire_vars.len(), NUM_WIRE_TYPES * self.domain_size);
        check(unsafe { capgpu_plonk_key_set_vars(self.handle, wire_vars.as_ptr(), num_vars) })
    }
    /// Length of a `prove_vars` witness; 0: the key has no table.
    pub fn num_vars(&self) -> Result<usize> {
        let mut nv = 0usize;
        check(unsafe { capgpu_plonk_key_num_vars(self.handle, &mut nv) })?;
        Ok(nv)
    }
    /// Names the variables the caller supplies (inputs, the constants 0 and 1, every hinted bit - not fifth roots); the
    /// key derives the schedule by which `solve` computes all the others.  Refused, naming the lowest offending row, when
    /// the circuit does not follow from the list by the rule of capgpu.h.
    pub fn set_given(&self, given_vars: &[u32]) -> Result<capgpu_solver_info> {
        let mut info = capgpu_solver_info::default();
        check(unsafe { capgpu_plonk_key_set_given(self.handle, given_vars.as_ptr(), given_vars.len(), &mut info) })?;
        Ok(info)
    }
    /// `set_given` with the hints the circuit's builder recorded (`capgpu_plonk_key_set_given_hints`): `targets` holds every
    /// hint's target ids, `hints[i].first` and `.count` its slice.  The hinted variables need not be given.
    pub fn set_given_hints(&self, given_vars: &[u32], hints: &[capgpu_hint], targets: &[u32])
                           -> Result<(capgpu_solver_info, capgpu_hint_info)> {
        let (mut info, mut hint_info) = (capgpu_solver_info::default(), capgpu_hint_info::default());
        check(unsafe {
            capgpu_plonk_key_set_given_hints(self.handle, given_vars.as_ptr(), given_vars.len(), hints.as_ptr(), hints.len(),
                                             targets.as_ptr(), targets.len(), &mut info, &mut hint_info)
        })?;
        Ok((info, hint_info))
    }
    /// `set_given_hints` under `flags` (`capgpu_plonk_key_set_solver`): `CAPGPU_SOLVER_LINEAR` admits rows that define their one
    /// unknown on an input wire through its linear selector - `enforce_equal(computed, public)` read backwards -,
    /// `CAPGPU_SOLVER_DERIVE_PUBLIC` lets public-input variables get their values from such rows instead of the list.
    /// `flags == 0` is `set_given_hints`.
    pub fn set_solver(&self, given_vars: &[u32], hints: &[capgpu_hint], targets: &[u32], flags: u32)
                      -> Result<(capgpu_solver_info, capgpu_hint_info)> {
        let (mut info, mut hint_info) = (capgpu_solver_info::default(), capgpu_hint_info::default());
        check(unsafe {
            capgpu_plonk_key_set_solver(self.handle, given_vars.as_ptr(), given_vars.len(), hints.as_ptr(), hints.len(),
                                        targets.as_ptr(), targets.len(), flags, &mut info, &mut hint_info)
        })?;
        Ok((info, hint_info))
    }
    /// The figures of the solver's flags: LIN rows and derived public inputs; all zero: no solver.
    pub fn solver_rules_info(&self) -> Result<capgpu_solver_rules_info> {
        let mut info = capgpu_solver_rules_info::default();
        check(unsafe { capgpu_plonk_key_solver_rules_info(self.handle, &mut info) })?;
        Ok(info)
    }
    /// Re-derives the schedule of the solver the key holds in `form` (`CAPGPU_SOLVE_FORM_DIRECT`, what every set-up call
    /// leaves, or `CAPGPU_SOLVE_FORM_DEFERRED`: a chain's denominators inverted together).  Same values, same statuses.
    pub fn set_solve_form(&self, form: c_int) -> Result<capgpu_solve_form_info> {
        let mut info = capgpu_solve_form_info::default();
        check(unsafe { capgpu_plonk_key_set_solve_form(self.handle, form, &mut info) })?;
        Ok(info)
    }
    /// The form the key's solver runs and its figures; all zero: no solver.
    pub fn solve_form_info(&self) -> Result<capgpu_solve_form_info> {
        let mut info = capgpu_solve_form_info::default();
        check(unsafe { capgpu_plonk_key_solve_form_info(self.handle, &mut info) })?;
        Ok(info)
    }
    /// The public inputs of `vars.len() / num_vars` completed assignments (what `solve` returns, or a `prove_vars` witness
    /// per assignment): per assignment the key's `num_inputs` values, for every row below num_inputs the value that makes
    /// the row hold.  The key needs a table, not a solver.  Both sizes come from the key: the library reads num_vars and
    /// writes num_inputs elements per assignment.
    pub fn pub_inputs(&self, vars: &[[u64; 4]]) -> Result<Vec<[u64; 4]>> {
        let nv = self.num_vars()?;
        assert!(nv > 0 && vars.len() % nv == 0, "pub_inputs: the key has no table, or vars is no multiple of num_vars");
        let count = vars.len() / nv;
        assert!(count <= c_int::MAX as usize);
        let mut out = vec![[0u64; 4]; count * self.num_inputs];
        check(unsafe {
            capgpu_plonk_pub_inputs(self.handle, count as c_int, vars.as_ptr() as *const u64, out.as_mut_ptr() as *mut u64)
        })?;
        Ok(out)
    }
    /// The figures of the key's hints; all zero: no hints.
    pub fn hint_info(&self) -> Result<capgpu_hint_info> {
        let mut info = capgpu_hint_info::default();
        check(unsafe { capgpu_plonk_key_hint_info(self.handle, &mut info) })?;
        Ok(info)
    }
    /// The schedule's figures; all zero: the key has no solver.
    pub fn solver_info(&self) -> Result<capgpu_solver_info> {
        let mut info = capgpu_solver_info::default();
        check(unsafe { capgpu_plonk_key_solver_info(self.handle, &mut info) })?;
        Ok(info)
    }
    /// Completes `given.len() / num_given` assignments on the device: `given` holds, per witness, the values of the
    /// given variables in the order of `set_given`'s list.  Returns the assignments (num_vars values each, ready for
    /// `prove_vars`) and one verdict per witness; `Ok` whenever the solve ran.
    pub fn solve(&self, given: &[[u64; 4]]) -> Result<(Vec<[u64; 4]>, Vec<capgpu_solve_status>)> {
        let per = self.solver_info()?.num_given as usize;
        let nv = self.num_vars()?;
        assert!(per > 0 && given.len() % per == 0);
        let count = given.len() / per;
        let mut vars = vec![[0u64; 4]; count * nv];
        let mut status = vec![capgpu_solve_status::default(); count];
        check(unsafe {
            capgpu_plonk_solve_vars(self.handle, count as c_int, given.as_ptr() as *const u64, vars.as_mut_ptr() as *mut u64,
                                    status.as_mut_ptr())
        })?;
        Ok((vars, status))
    }
    /// The same proof from the circuit's variable assignment (`CAPGPU_INPUT_VARS`): `witness` = `circuit.witness`, one
    /// value per variable - an eighth of the bytes of the five columns for a CAP transfer; the columns are gathered on
    /// the device through the key's table.  Same proof bytes as `prove` on the expanded columns.
    pub fn prove_vars(&self, witness: &[[u64; 4]], pub_inputs: &[[u64; 4]], ext_msg: &[u8], blinders: &[[u64; 4]; 13]) -> Result<capgpu_proof> {
        assert_eq!(witness.len(), self.num_vars()?);
        assert_eq!(pub_inputs.len(), self.num_inputs);
        let mut proof: capgpu_proof = unsafe { std::mem::zeroed() };
        check(unsafe {
            capgpu_plonk_prove_ex(self.handle, witness.as_ptr() as *const u64, pub_inputs.as_ptr() as *const u64,
                                  pub_inputs.len(), ext_msg.as_ptr(), ext_msg.len(), blinders.as_ptr() as *const u64,
                                  CAPGPU_INPUT_VARS, &mut proof)
        })?;
        Ok(proof)
    }
    /// `PlonkKzgSnark::prove::<_, _, SolidityTranscript>(rng, circuit, pk, Some(ext_msg))` for one note: callable from
    /// any thread; with coalescing on, concurrent calls share device batches.  `wires`: the 5 finalised wire COLUMNS, n
    /// VALUES each (`CAPGPU_INPUT_EVALS` - what this name has always taken); `blinders`: 13 `Fr::rand(rng)` draws in
    /// jf-plonk's order (2 per wire polynomial, then 3).
    pub fn prove(&self, wires: &[[u64; 4]], pub_inputs: &[[u64; 4]], ext_msg: &[u8], blinders: &[[u64; 4]; 13]) -> Result<capgpu_proof> {
        self.prove_form(wires, pub_inputs, ext_msg, blinders, CAPGPU_INPUT_EVALS)
    }
    /// The same from the 5 UNBLINDED wire POLYNOMIALS, n coefficients each (`CAPGPU_INPUT_COEFFS`) -
    /// `arkworks::poly_columns(&circuit.compute_wire_polynomials()?, n)`: what a jf-relation caller holds.  Same proof
    /// bytes as `prove` on the values.
    pub fn prove_coeffs(&self, wire_polys: &[[u64; 4]], pub_inputs: &[[u64; 4]], ext_msg: &[u8], blinders: &[[u64; 4]; 13]) -> Result<capgpu_proof> {
        self.prove_form(wire_polys, pub_inputs, ext_msg, blinders, CAPGPU_INPUT_COEFFS)
    }
    /// Either form, stated explicitly.
    pub fn prove_form(&self, wires: &[[u64; 4]], pub_inputs: &[[u64; 4]], ext_msg: &[u8], blinders: &[[u64; 4]; 13],
                      input_form: c_int) -> Result<capgpu_proof> {
        assert_eq!(wires.len(), NUM_WIRE_TYPES * self.domain_size);
        assert_eq!(pub_inputs.len(), self.num_inputs);
        let mut proof: capgpu_proof = unsafe { std::mem::zeroed() };
        check(unsafe {
            capgpu_plonk_prove_ex(self.handle, wires.as_ptr() as *const u64, pub_inputs.as_ptr() as *const u64,
                                  pub_inputs.len(), ext_msg.as_ptr(), ext_msg.len(), blinders.as_ptr() as *const u64,
                                  input_form, &mut proof)
        })?;
        Ok(proof)
    }
    /// Starts proving `proofs.len()` notes from host memory and returns at once: the ticket borrows the witnesses, public
    /// inputs, blinders and the output slice for its lifetime, `wait()` - or its `Drop` - ends the borrow.  A `Vec` of
    /// notes is proved from ONE thread by keeping two tickets in flight: no rayon pool, no
    /// `capgpu_set_device`.  `wires`: per proof the 5 columns of n values (or coefficients, `input_form`), consecutive;
    /// `blinders`: 13 per proof.  `CAPGPU_ERR_BUSY`: 64 tickets outstanding - wait for one and submit again.
    pub fn prove_batch_async<'a>(&self, wires: &'a [[u64; 4]], pub_inputs: &'a [[u64; 4]], ext_msg: &[u8],
                                 blinders: &'a [[u64; 4]], input_form: c_int, proofs: &'a mut [capgpu_proof])
                                 -> Result<ProveTicket<'a>> {
        let count = proofs.len();
        let per = if input_form == CAPGPU_INPUT_VARS { self.num_vars()? } else { NUM_WIRE_TYPES * self.domain_size };
        assert_eq!(wires.len(), count * per);
        assert_eq!(pub_inputs.len(), count * self.num_inputs);
        assert_eq!(blinders.len(), count * 13);
        let mut ticket = 0u64;
        check(unsafe {
            capgpu_plonk_prove_batch_async(self.handle, count as c_int, wires.as_ptr() as *const u64,
                                           pub_inputs.as_ptr() as *const u64, self.num_inputs, ext_msg.as_ptr(),
                                           ext_msg.len(), blinders.as_ptr() as *const u64, input_form,
                                           proofs.as_mut_ptr(), &mut ticket)
        })?;
        Ok(ProveTicket { ticket, done: false, _borrow: std::marker::PhantomData })
    }
    /// One `prove()` per note with a `Result` of its own - the reference's rayon map over a `Vec` of notes
    /// (src/utils/params_builder.rs:194-226) - as ONE device batch under this key (`capgpu_plonk_prove_each`): a note
    /// whose witness does not satisfy the circuit gets `Err(ProveError)` with the message its own `prove` would give and
    /// costs the others nothing; an `Ok` proof is bit for bit `prove_form`'s.  The outer `Err`: the batch could not run.
    /// `wires`, `pub_inputs`, `blinders`: per proof, consecutive (as `prove_batch_async`); `ext_msgs`: one per proof.
    pub fn prove_each(&self, wires: &[[u64; 4]], pub_inputs: &[[u64; 4]], ext_msgs: &[&[u8]], blinders: &[[u64; 4]],
                      input_form: c_int) -> Result<Vec<std::result::Result<capgpu_proof, ProveError>>> {
        let count = ext_msgs.len();
        let per = if input_form == CAPGPU_INPUT_VARS { self.num_vars()? } else { NUM_WIRE_TYPES * self.domain_size };
        assert_eq!(wires.len(), count * per);
        assert_eq!(pub_inputs.len(), count * self.num_inputs);
        assert_eq!(blinders.len(), count * 13);
        let handles = vec![self.handle; count];
        let msgs: Vec<*const u8> = ext_msgs.iter().map(|m| if m.is_empty() { std::ptr::null() } else { m.as_ptr() }).collect();
        let lens: Vec<usize> = ext_msgs.iter().map(|m| m.len()).collect();
        let mut proofs: Vec<capgpu_proof> = (0..count).map(|_| unsafe { std::mem::zeroed() }).collect();
        let mut outcomes = vec![capgpu_prove_outcome::default(); count];
        check(unsafe {
            capgpu_plonk_prove_each(handles.as_ptr(), count as c_int, wires.as_ptr() as *const u64,
                                    pub_inputs.as_ptr() as *const u64, self.num_inputs, msgs.as_ptr(), lens.as_ptr(),
                                    blinders.as_ptr() as *const u64, input_form, proofs.as_mut_ptr(),
                                    outcomes.as_mut_ptr())
        })?;
        Ok(proofs.into_iter().zip(outcomes).map(|(p, o)| if o.status == CAPGPU_OK { Ok(p) } else { Err(ProveError::from(o)) })
            .collect())
    }
    /// `prove()` for ONE note from the values its circuit is given (`capgpu_plonk_prove_given_one`): the call of a rayon
    /// map over notes - `notes.par_iter().map(|n| pk.prove_given_one(..)).collect::<Vec<_>>()`.  With `set_coalescing`
    /// on, the concurrent calls are gathered into one solve and one device batch; every caller's `Ok` proof is bit for bit
    /// its lone call's.  `Err`: the outcome record and message of a witness that does not satisfy the circuit, or - a
    /// call that could not run - the library's code in `outcome.status` and its message.
    pub fn prove_given_one(&self, given: &[[u64; 4]], pub_inputs: &[[u64; 4]], ext_msg: &[u8], blinders: &[[u64; 4]; 13])
                           -> std::result::Result<capgpu_proof, ProveError> {
        let mut proof: capgpu_proof = unsafe { std::mem::zeroed() };
        let mut outcome = capgpu_prove_outcome::default();
        let rc = unsafe {
            capgpu_plonk_prove_given_one(self.handle, given.as_ptr() as *const u64, given.len(),
                                         pub_inputs.as_ptr() as *const u64, pub_inputs.len(),
                                         if ext_msg.is_empty() { std::ptr::null() } else { ext_msg.as_ptr() }, ext_msg.len(),
                                         blinders.as_ptr() as *const u64, &mut proof, &mut outcome, std::ptr::null_mut())
        };
        if let Err(e) = check(rc) {
            outcome.status = e.code;
            return Err(ProveError { outcome, message: e.message });
        }
        if outcome.status == CAPGPU_OK { Ok(proof) } else { Err(ProveError::from(outcome)) }
    }
    /// Sizes context `slot` (-1: every context) ahead for batches of `count` host-resident proofs under this key, so that
    /// no allocation lands inside a steady-state call (`scratch_stats` then stays put).
    pub fn reserve(&self, count: usize, input_form: c_int, slot: i32) -> Result<()> {
        check(unsafe { capgpu_plonk_reserve(self.handle, count as c_int, input_form, slot) })
    }
    pub fn handle(&self) -> u64 {
        self.handle
    }
}
/// One note of `prove_notes`: its key, its own witness block (5 n elements, or - `CAPGPU_INPUT_VARS` - the key's num_vars
/// values), the public inputs of ITS key, its transcript message and its blinders.
pub struct Note<'a> {
    pub key: &'a ProvingKey,
    pub wires: &'a [[u64; 4]],
    pub pub_inputs: &'a [[u64; 4]],
    pub ext_msg: &'a [u8],
    pub blinders: &'a [[u64; 4]; 13],
}
/// The reference's `Vec<TransactionNote>` of transfers, mints and freezes - keys of SEVERAL domain sizes - proved in ONE
/// call (`capgpu_plonk_prove_notes`): every note gets a `Result` of its own, bit for bit what `ProvingKey::prove_each`
/// makes of the notes of its group (same domain size and SRS) alone.  The witness blocks are read where they are.
pub fn prove_notes(notes: &[Note<'_>], input_form: c_int) -> Result<Vec<std::result::Result<capgpu_proof, ProveError>>> {
    let count = notes.len();
    let num_inputs = notes.iter().map(|n| n.key.num_inputs).max().unwrap_or(0);
    let handles: Vec<u64> = notes.iter().map(|n| n.key.handle).collect();
    let rows: Vec<*const u64> = notes.iter().map(|n| n.wires.as_ptr() as *const u64).collect();
    let mut pubs = vec![[0u64; 4]; count * num_inputs];
    let mut blinders = Vec::with_capacity(count * 13);
    for (i, n) in notes.iter().enumerate() {
        assert_eq!(n.pub_inputs.len(), n.key.num_inputs);
        pubs[i * num_inputs..i * num_inputs + n.pub_inputs.len()].copy_from_slice(n.pub_inputs);
        blinders.extend_from_slice(&n.blinders[..]);
    }
    let msgs: Vec<*const u8> = notes.iter().map(|n| if n.ext_msg.is_empty() { std::ptr::null() } else { n.ext_msg.as_ptr() }).collect();
    let lens: Vec<usize> = notes.iter().map(|n| n.ext_msg.len()).collect();
    let mut proofs: Vec<capgpu_proof> = (0..count).map(|_| unsafe { std::mem::zeroed() }).collect();
    let mut outcomes = vec![capgpu_prove_outcome::default(); count];
    check(unsafe {
        capgpu_plonk_prove_notes(handles.as_ptr(), count as c_int, rows.as_ptr(), pubs.as_ptr() as *const u64, num_inputs,
                                 msgs.as_ptr(), lens.as_ptr(), blinders.as_ptr() as *const u64, input_form,
                                 proofs.as_mut_ptr(), outcomes.as_mut_ptr())
    })?;
    Ok(proofs.into_iter().zip(outcomes).map(|(p, o)| if o.status == CAPGPU_OK { Ok(p) } else { Err(ProveError::from(o)) })
        .collect())
}
/// Why one note of `ProvingKey::prove_each` has no proof: the outcome record and `capgpu_prove_outcome_text` of it.
#[derive(Clone)]
pub struct ProveError {
    pub outcome: capgpu_prove_outcome,
    pub message: String,
}
impl From<capgpu_prove_outcome> for ProveError {
    fn from(outcome: capgpu_prove_outcome) -> Self {
        let mut buf = [0 as c_char; 512];
        unsafe { capgpu_prove_outcome_text(&outcome, buf.as_mut_ptr(), buf.len()) };
        let message = unsafe { std::ffi::CStr::from_ptr(buf.as_ptr()) }.to_string_lossy().into_owned();
        ProveError { outcome, message }
    }
}
impl std::fmt::Display for ProveError {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        write!(f, "{}", self.message)
    }
}
impl Drop for ProvingKey {
    fn drop(&mut self) {
        unsafe { capgpu_plonk_free_key(self.handle) };
    }
}

/// A batch being proved by a worker thread of the library (`ProvingKey::prove_batch_async`).  It holds the borrows of the
/// input slices and of the output slice: the compiler keeps the caller from touching `proofs` - or freeing the witnesses -
/// until the ticket is gone, which is what the C ABI asks for.  Dropping a ticket waits for it.
pub struct ProveTicket<'a> {
    ticket: u64,
    done: bool,
    _borrow: std::marker::PhantomData<&'a mut [capgpu_proof]>,
}
impl<'a> ProveTicket<'a> {
    /// Blocks until the batch is proved; the proving call's error, if any, is the result.
    pub fn wait(mut self) -> Result<()> {
        self.wait_inner(u32::MAX).map(|_| ())
    }
    /// `Ok(true)`: done (the proofs are in the output slice once the ticket is dropped); `Ok(false)`: not yet.
    pub fn wait_timeout(&mut self, timeout_ms: u32) -> Result<bool> {
        self.wait_inner(timeout_ms)
    }
    fn wait_inner(&mut self, timeout_ms: u32) -> Result<bool> {
        if self.done {
            return Ok(true);
        }
        let mut done: c_int = 0;
        let rc = unsafe { capgpu_wait(self.ticket, timeout_ms, &mut done) };
        if rc != CAPGPU_OK || done != 0 {
            self.done = true; // consumed (or unknown to the library: nothing is borrowed any more)
        }
        check(rc)?;
        Ok(done != 0)
    }
}
impl<'a> Drop for ProveTicket<'a> {
    fn drop(&mut self) {
        if !self.done {
            let mut done: c_int = 0;
            unsafe { capgpu_wait(self.ticket, u32::MAX, &mut done) };
        }
    }
}

/// The 769 ark-serialize bytes of a proof as it sits inside a `TransferNote` (src/transfer.rs:54-66).
pub fn proof_bytes(proof: &capgpu_proof) -> Result<Vec<u8>> {
    let mut out = vec![0u8; 1024];
    let mut len = 0usize;
    check(unsafe { capgpu_proof_serialize(proof, out.as_mut_ptr(), out.len(), &mut len) })?;
    out.truncate(len);
    Ok(out)
}

/// Bytes of one serialized proof (`CAPGPU_PROOF_BYTES`).
pub const PROOF_BYTES: usize = 769;

/// `Proof::deserialize` for a block of notes on the device: `records` holds one `PROOF_BYTES` record per proof, packed.
/// A record that does not decode is not an error: its status is 1 + the byte offset of the first malformed field (0:
/// decoded) and its proof is all-ones words, which every verifier of the library refuses.
pub fn proofs_from_bytes(records: &[u8]) -> Result<(Vec<capgpu_proof>, Vec<c_int>)> {
    assert!(records.len() % PROOF_BYTES == 0, "not a whole number of proof records");
    let count = records.len() / PROOF_BYTES;
    let mut proofs: Vec<capgpu_proof> = Vec::with_capacity(count);
    let mut status = vec![0 as c_int; count];
    check(unsafe { capgpu_proof_decode_batch(records.as_ptr(), PROOF_BYTES, count, proofs.as_mut_ptr(), status.as_mut_ptr()) })?;
    unsafe { proofs.set_len(count) }; // every struct was written by the call
    Ok((proofs, status))
}

/// The inverse: the note bytes of a batch of proofs (`capgpu_proof_serialize` for each), packed.
pub fn proofs_to_bytes(proofs: &[capgpu_proof]) -> Result<Vec<u8>> {
    let mut out = vec![0u8; proofs.len() * PROOF_BYTES];
    check(unsafe { capgpu_proof_encode_batch(proofs.as_ptr(), proofs.len(), out.as_mut_ptr(), PROOF_BYTES) })?;
    Ok(out)
}

/// `txn_batch_verify` (src/lib.rs:455-529) for a validator that holds each note's proof as its bytes: keys uploaded once
/// (`capgpu_plonk_vk_upload`), `records` as above, `pub_inputs` one row of `num_inputs` elements per proof, `ext_msgs`
/// empty or one message per proof.  Decoding and verification run on the device behind one host wait.  `Ok(true)`: every
/// proof of the block holds; a record that does not decode makes it `Ok(false)` like any wrong proof.
pub fn verify_block_bytes(vk_handles: &[u64], g2_h: &[u64; 16], g2_beta_h: &[u64; 16], pub_inputs: &[[u64; 4]],
                          num_inputs: usize, records: &[u8], ext_msgs: &[&[u8]]) -> Result<bool> {
    let count = vk_handles.len();
    assert!(records.len() == count * PROOF_BYTES && pub_inputs.len() == count * num_inputs);
    assert!(ext_msgs.is_empty() || ext_msgs.len() == count);
    let msgs: Vec<*const u8> = ext_msgs.iter().map(|m| if m.is_empty() { std::ptr::null() } else { m.as_ptr() }).collect();
    let lens: Vec<usize> = ext_msgs.iter().map(|m| m.len()).collect();
    let mut ok: c_int = 0;
    check(unsafe {
        capgpu_plonk_verify_block_bytes(vk_handles.as_ptr(), g2_h.as_ptr(), g2_beta_h.as_ptr(),
                                        if pub_inputs.is_empty() { std::ptr::null() } else { pub_inputs.as_ptr() as *const u64 },
                                        num_inputs, records.as_ptr(), PROOF_BYTES,
                                        if msgs.is_empty() { std::ptr::null() } else { msgs.as_ptr() },
                                        if lens.is_empty() { std::ptr::null() } else { lens.as_ptr() }, count, &mut ok,
                                        std::ptr::null_mut(), std::ptr::null_mut())
    })?;
    Ok(ok != 0)
}

/// Conversions between arkworks 0.3 values and the ABI's words, and the circuit columns from jf-relation's PUBLIC API.
/// [DEP-RECALLED: written from the crates' APIs at the pinned revisions; this module has never been compiled.]
#[cfg(feature = "arkworks")]
pub mod arkworks {
    use ark_bn254::{Fq, Fr, G1Projective};
    use ark_ff::{BigInteger256, PrimeField};
    use ark_poly::univariate::DensePolynomial;

    /// `Fp256` keeps its Montgomery limbs in `.0.0`: the ABI's "Montgomery words".
    pub fn fr_words(x: &Fr) -> [u64; 4] {
        (x.0).0
    }
    pub fn fr_from_words(w: [u64; 4]) -> Fr {
        Fr::new(BigInteger256(w))
    }
    /// canonical integer of a scalar (`into_repr()`): what the MSM takes
    pub fn fr_canonical(x: &Fr) -> [u64; 4] {
        x.into_repr().0
    }
    /// (X, Y, Z) Montgomery words -> `GroupProjective` (Z = 0: the identity)
    pub fn g1_from_xyz(w: &[u64; 12]) -> G1Projective {
        let f = |i: usize| Fq::new(BigInteger256([w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]]));
        G1Projective::new(f(0), f(1), f(2))
    }
    /// A family of polynomials as the ABI's coefficient-form columns (`CAPGPU_INPUT_COEFFS`): n coefficients each,
    /// column-major, a `DensePolynomial` shorter than n (arkworks strips trailing zeros) zero-padded.  jf-relation's
    /// `Arithmetization` trait hands the prover exactly these polynomials, so nothing is transformed on the CPU:
    ///   let n = circuit.eval_domain_size()?;
    ///   let selectors = poly_columns(&circuit.compute_selector_polynomials()?, n);              // 13 x n
    ///   let sigma     = poly_columns(&circuit.compute_extended_permutation_polynomials()?, n);  // 5 x n
    ///   let wires     = poly_columns(&circuit.compute_wire_polynomials()?, n);                  // 5 x n (per proof)
    /// A memcpy of 5 n field elements per proof - against the 10 n-point FFTs per proof the evaluation form used to
    /// cost this shim (5 here to undo jf-relation's interpolation, 5 on the device to redo it).
    pub fn poly_columns(polys: &[DensePolynomial<Fr>], n: usize) -> Vec<[u64; 4]> {
        let mut out = vec![[0u64; 4]; polys.len() * n];
        for (i, p) in polys.iter().enumerate() {
            assert!(p.coeffs.len() <= n, "polynomial longer than the evaluation domain");
            for (j, c) in p.coeffs.iter().enumerate() {
                out[i * n + j] = fr_words(c);
            }
        }
        out
    }
    /// The evaluation-form columns (`CAPGPU_INPUT_EVALS`) of a family of polynomials: one n-point FFT each on the CPU.
    /// Kept for callers written against rounds 1-3 of this crate; new code passes `poly_columns` to the `_coeffs` entry
    /// points and lets the device do the transform.
    #[deprecated(note = "pass poly_columns(..) to preprocess_coeffs / prove_coeffs instead: no CPU transform")]
    pub fn circuit_columns(polys: &[DensePolynomial<Fr>], n: usize) -> Vec<[u64; 4]> {
        use ark_poly::{EvaluationDomain, Radix2EvaluationDomain};
        let domain = Radix2EvaluationDomain::<Fr>::new(n).expect("power-of-two domain");
        let mut out = vec![[0u64; 4]; polys.len() * n];
        for (i, p) in polys.iter().enumerate() {
            for (j, v) in domain.fft(&p.coeffs).iter().enumerate() {
                out[i * n + j] = fr_words(v);
            }
        }
        out
    }
}
