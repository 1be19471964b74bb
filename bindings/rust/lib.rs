//! Safe Rust wrapper over `libbfhip.so` — the whole-path entry points of the MI355X backend (source only: the build image has no
//! Rust toolchain). `bfhip_sys.rs` is generated from `include/bfhip.h` by `tools/gen_rust_ffi.py`.
//!
//! In `crates/brainfuck_prover` this replaces the body of `prove_brainfuck` (`brainfuck_air/mod.rs:471`):
//! ```ignore
//! let ctx = bfhip::Context::new(0, LOG_MAX_ROWS + 2)?;
//! let json = ctx.prove_brainfuck(&code, &input, LOG_MAX_ROWS)?;
//! let proof: BrainfuckProof<Blake2sMerkleHasher> = serde_json::from_slice(&json)?;   // same serde shape (mod.rs:71-99)
//! ```
#[path = "bfhip_sys.rs"]
pub mod sys;
/// stwo's backend trait surface (`Backend`, `ColumnOps`, `FieldOps`, `PolyOps`, `MerkleOps`, `QuotientOps`, `FriOps`, `AccumulationOps`, `GrindOps`,
/// `ComponentProver`) over the FFI — for `prover::prove::<HipBackend, _>` at `mod.rs:732`.
/// Never compiled (no toolchain, stwo not vendored): kept out of the default module tree behind the feature `stwo-backend`.
#[cfg(feature = "stwo-backend")]
#[path = "hip_backend.rs"]
pub mod hip_backend;

use std::ffi::{c_char, c_void, CStr, CString};

fn last_error() -> String {
    unsafe { CStr::from_ptr(sys::bfhip_last_error()).to_string_lossy().into_owned() }
}

/// One GPU + one HIP stream + the twiddle tree (`mod.rs:480-487`). Calls on a context are serial.
pub struct Context(*mut sys::BfhipCtx);

// A context may be moved to another thread; every entry point binds the calling thread to the context's GPU.
unsafe impl Send for Context {}

impl Context {
    pub fn new(device_id: i32, max_log_domain: u32) -> Result<Self, String> {
        let mut p = std::ptr::null_mut();
        if unsafe { sys::bfhip_ctx_create(device_id, max_log_domain, &mut p) } != 0 {
            return Err(last_error());
        }
        Ok(Context(p))
    }

    /// `prove_brainfuck` (`mod.rs:471-735`): compile, run, build the tables, commit, prove. Returns the serde-JSON proof bytes.
    pub fn prove_brainfuck(&self, code: &str, input: &[u8], log_max_rows: u32) -> Result<Vec<u8>, String> {
        let code = CString::new(code).map_err(|e| e.to_string())?;
        let (mut js, mut len): (*mut c_char, usize) = (std::ptr::null_mut(), 0);
        let rc = unsafe {
            sys::bfhip_prove_brainfuck(self.0, code.as_ptr(), input.as_ptr(), input.len(), log_max_rows, &mut js, &mut len,
                                       std::ptr::null_mut(), std::ptr::null_mut())
        };
        if rc != 0 {
            return Err(last_error());   // "ConstraintsNotSatisfied", "a component exceeds LOG_MAX_ROWS", HIP errors, ...
        }
        let out = unsafe { std::slice::from_raw_parts(js as *const u8, len) }.to_vec();
        unsafe { sys::bfhip_free_host(js as *mut c_void) };
        Ok(out)
    }

    /// `prove_brainfuck(&Machine)` as the reference receives it (`mod.rs:471-473`): the executed machine's register trace
    /// (`inputs.trace()`, `mod.rs:508`; 7 words per row: clk, ip, ci, ni, mp, mv, mvi) and its program words — no re-execution, and ONE
    /// call (`bfhip_prove_registers`): the rows are transposed and checked on the GPU while it already commits the preprocessed tree, and no
    /// resident trace is created. A non-canonical register is an `Err` that names its (row, register).
    pub fn prove_machine(&self, trace7: &[u32], program: &[u32], log_max_rows: u32) -> Result<Vec<u8>, String> {
        assert!(trace7.len() % 7 == 0);
        let (mut js, mut len): (*mut c_char, usize) = (std::ptr::null_mut(), 0);
        let rc = unsafe {
            sys::bfhip_prove_registers(self.0, trace7.as_ptr(), trace7.len() / 7, program.as_ptr(), program.len(), log_max_rows, &mut js, &mut len,
                                       std::ptr::null_mut(), std::ptr::null_mut())
        };
        if rc != 0 {
            return Err(last_error());
        }
        let out = unsafe { std::slice::from_raw_parts(js as *const u8, len) }.to_vec();
        unsafe { sys::bfhip_free_host(js as *mut c_void) };
        Ok(out)
    }

    /// `assert_constraints` for an executed machine (`bfhip_trace_check`): the 13 AIRs asserted on the trace domain, logUp columns generated
    /// with the default lookup elements of `include/bfhip.h`. `Ok(reports)` = every constraint holds on every row and the 13 claimed sums
    /// cancel (`lookup_sum_valid`, `mod.rs:207-226`); `Err` names the first failing component, constraint and table row — where a proof of
    /// the same trace would only say "ConstraintsNotSatisfied".
    pub fn check_machine(&self, trace7: &[u32], program: &[u32]) -> Result<[sys::BfhipCheckReport; 13], String> {
        assert!(trace7.len() % 7 == 0);
        let mut tr: *mut sys::BfhipTrace = std::ptr::null_mut();
        let rc = unsafe {
            sys::bfhip_trace_create_from_registers(self.0, trace7.as_ptr(), trace7.len() / 7, program.as_ptr(), program.len(), &mut tr, std::ptr::null_mut(),
                                                   std::ptr::null_mut(), std::ptr::null_mut())
        };
        if rc != 0 {
            return Err(last_error());
        }
        let mut reports = [sys::BfhipCheckReport::default(); 13];
        let (mut total, mut n_bad) = ([0u32; 4], 0i32);
        let rc = unsafe { sys::bfhip_trace_check(self.0, tr, std::ptr::null(), reports.as_mut_ptr(), total.as_mut_ptr(), &mut n_bad) };
        unsafe { sys::bfhip_trace_destroy(self.0, tr) };
        if rc != 0 {
            return Err(last_error());
        }
        if let Some(r) = reports.iter().find(|r| r.n_bad_cells != 0) {
            let j = r.first_bad_constraint as usize;
            return Err(format!("component {}: constraint {} fails at table row {} (cell {}), value {:?}; {} cells violate it",
                               r.component, j, r.first_bad_cell >> 4, r.first_bad_cell, r.first_bad_value, r.bad_per_constraint[j]));
        }
        if total != [0u32; 4] {
            return Err(format!("the 13 claimed logUp sums add up to {:?}, not zero", total));
        }
        Ok(reports)
    }

    /// stwo's relation tracker for an executed machine (`bfhip_trace_relations`): the counts of the three lookup relations (Memory,
    /// Instruction, Processor) and, per relation, up to `max_entries` tuples whose multiplicities do not cancel — what lies behind a non-zero
    /// logUp total of `check_machine`. Table index = component; counts are per table row (16 trace cells each).
    pub fn relations(&self, trace7: &[u32], program: &[u32], max_entries: u32) -> Result<([sys::BfhipRelationReport; 3], Vec<sys::BfhipRelationEntry>), String> {
        assert!(trace7.len() % 7 == 0);
        let mut tr: *mut sys::BfhipTrace = std::ptr::null_mut();
        let rc = unsafe {
            sys::bfhip_trace_create_from_registers(self.0, trace7.as_ptr(), trace7.len() / 7, program.as_ptr(), program.len(), &mut tr, std::ptr::null_mut(),
                                                   std::ptr::null_mut(), std::ptr::null_mut())
        };
        if rc != 0 {
            return Err(last_error());
        }
        let mut reports = [sys::BfhipRelationReport::default(); 3];
        let mut entries = vec![sys::BfhipRelationEntry::default(); 3 * max_entries as usize];
        let entries_ptr = if max_entries == 0 { std::ptr::null_mut() } else { entries.as_mut_ptr() };
        let rc = unsafe { sys::bfhip_trace_relations(self.0, tr, reports.as_mut_ptr(), entries_ptr, max_entries) };
        unsafe { sys::bfhip_trace_destroy(self.0, tr) };
        if rc != 0 {
            return Err(last_error());
        }
        let mut listed = Vec::new();
        for (r, rep) in reports.iter().enumerate() {
            listed.extend_from_slice(&entries[r * max_entries as usize..r * max_entries as usize + rep.n_reported as usize]);
        }
        Ok((reports, listed))
    }

    /// Byte-level stwo conventions / Merkle channel of this context (`bfhip_conventions`; all zero = defaults).
    pub fn set_conventions(&self, conv: &sys::BfhipConventions) -> Result<(), String> {
        if unsafe { sys::bfhip_ctx_set_conventions(self.0, conv) } != 0 { Err(last_error()) } else { Ok(()) }
    }

    /// Keep the program-independent preprocessed tree across proofs (the reference recommits it in every call).
    pub fn reuse_preprocessed(&self, on: bool) {
        unsafe { sys::bfhip_ctx_reuse_preprocessed(self.0, on as i32) };
    }

    /// The proof's own filter (`bfhip_ctx_set_preflight`): every later `prove_*` of this context first asserts the 13 AIRs and the logUp total
    /// on its tables and fails with the rejection lines ("TraceRejected: ...", then component / row / tuple) — the C status is
    /// `sys::BFHIP_TRACE_REJECTED`, `bfhip_ctx_last_preflight` has the report — instead of proving a trace that cannot be proved. A filter,
    /// not a soundness gate: its lookup elements are fixed and public. Refused for a context in a shard group.
    pub fn set_preflight(&self, on: bool) -> Result<(), String> {
        if unsafe { sys::bfhip_ctx_set_preflight(self.0, on as i32) } != 0 { Err(last_error()) } else { Ok(()) }
    }

    /// Device memory of this context in bytes: [reserved by the per-proof arena, its peak use, the twiddle trees, in use now] (`bfhip_ctx_memory`).
    pub fn memory(&self) -> Result<[u64; 4], String> {
        let mut out = [0u64; 4];
        if unsafe { sys::bfhip_ctx_memory(self.0, out.as_mut_ptr()) } != 0 { Err(last_error()) } else { Ok(out) }
    }
}

impl Drop for Context {
    fn drop(&mut self) {
        unsafe { sys::bfhip_ctx_destroy(self.0) };
    }
}

/// What `prove_brainfuck(&Machine)` reads of an executed machine (`mod.rs:471-473`, `:508`): `inputs.trace()` flattened to 7 words per row
/// (clk, ip, ci, ni, mp, mv, mvi) and `inputs.program()` as words. Build it once per machine; a pool borrows it until the result is taken.
pub struct Machine {
    pub trace7: Vec<u32>,
    pub program: Vec<u32>,
}

/// One finished job of a pool's queue (`bfhip_pool_result`).
pub struct JobResult {
    pub ticket: u64,
    pub tag: u64,
    /// the sub-context that ran the job
    pub worker: u32,
    /// `bfhip_ctx_last_proof_flags` of that proof (bit 2: it read the pool's shared preprocessed tree)
    pub flags: u32,
    pub seconds_queued: f64,
    pub seconds_proving: f64,
    /// the proof's serde-JSON bytes, or the job's own error text ("job <ticket>: ..."; `cancelled` tells a cancelled job from a failed one)
    pub proof: Result<Vec<u8>, String>,
    pub cancelled: bool,
}

/// `bfhip_pool_*`: k proofs in flight on one GPU behind a queue. `submit_machine` returns at once with a ticket, `wait` hands out results in
/// completion order. The lifetime ties every submitted machine to the pool: the library borrows the register rows until the job's result
/// has been taken, and dropping the pool lets running jobs finish first.
pub struct Pool<'a> {
    ptr: *mut sys::BfhipPool,
    log_max_rows: u32,
    _machines: std::marker::PhantomData<&'a Machine>,
}

// One producer thread may submit while one consumer thread waits (include/bfhip.h).
unsafe impl<'a> Send for Pool<'a> {}
unsafe impl<'a> Sync for Pool<'a> {}

impl<'a> Pool<'a> {
    pub fn new(device_id: i32, n_in_flight: u32, log_max_rows: u32) -> Result<Self, String> {
        let mut p = std::ptr::null_mut();
        if unsafe { sys::bfhip_pool_create(device_id, n_in_flight, log_max_rows + 2, &mut p) } != 0 {
            return Err(last_error());
        }
        Ok(Pool { ptr: p, log_max_rows, _machines: std::marker::PhantomData })
    }

    /// `bfhip_pool_submit_registers`: queues the proof of an executed machine and returns its ticket. `Err` = the submit itself was refused
    /// (empty trace, 4096 jobs outstanding); everything else comes back as that job's result.
    pub fn submit_machine(&self, machine: &'a Machine, tag: u64) -> Result<u64, String> {
        assert!(machine.trace7.len() % 7 == 0);
        let mut ticket = 0u64;
        let rc = unsafe {
            sys::bfhip_pool_submit_registers(self.ptr, machine.trace7.as_ptr(), machine.trace7.len() / 7, machine.program.as_ptr(), machine.program.len(),
                                             self.log_max_rows, tag, &mut ticket)
        };
        if rc != 0 { Err(last_error()) } else { Ok(ticket) }
    }

    /// `bfhip_pool_submit_air`: what `air_prove` takes, as a job; the result's proof is `air_prove`'s bytes. The library copies the statement,
    /// the table of column pointers and the channel's state at submit: `channel` is not advanced. It borrows the programs and the kernels
    /// until the job's result has been taken — the lifetime `'a` keeps them alive as long as the pool — and the device columns behind
    /// `tree_cols`, which the caller must not free before then. `kernels`: empty, or `n_in_flight * n_components` entries, row w = the
    /// kernels compiled on sub-context w. `Err` = the submit itself was refused (the validator's rule, other conventions, 4096 outstanding).
    pub fn submit_air(&self, statement: &AirStatement<'a>, tree_cols: &[&[*const u32]], kernels: &[Option<&'a AirKernel>], channel: &Channel, check_trace: bool,
                      tag: u64) -> Result<u64, String> {
        if tree_cols.len() != statement.trees.len() || tree_cols.iter().zip(statement.trees.iter()).any(|(c, t)| c.len() != t.log_sizes.len()) {
            return Err("one device column per column of every caller tree".into());
        }
        let mut n_in_flight = 0u32;
        check(unsafe { sys::bfhip_pool_size(self.ptr, &mut n_in_flight) })?;
        if !kernels.is_empty() && kernels.len() != n_in_flight as usize * statement.components.len() {
            return Err("n_in_flight rows of one kernel (or None) per component".into());
        }
        let raw = statement.raw();
        let trees: Vec<*const *const u32> = tree_cols.iter().map(|c| c.as_ptr()).collect();
        let ks: Vec<*mut sys::BfhipAirKernel> = kernels.iter().map(|k| k.map_or(std::ptr::null_mut(), |k| k.0)).collect();
        let mut ticket = 0u64;
        let rc = unsafe {
            sys::bfhip_pool_submit_air(self.ptr, &raw.st, trees.as_ptr(), if ks.is_empty() { std::ptr::null() } else { ks.as_ptr() }, channel.0 as *const sys::BfhipChannel,
                                       if check_trace { sys::BFHIP_AIR_PROVE_CHECK } else { 0 }, tag, &mut ticket)
        };
        if rc != 0 { Err(last_error()) } else { Ok(ticket) }
    }

    /// `bfhip_pool_wait`: `Ok(Some(result))`, `Ok(None)` when nothing is outstanding, `Err("timeout")` when `timeout_ms` (`u32::MAX` = no
    /// limit, 0 = poll) ran out with jobs outstanding.
    pub fn wait(&self, timeout_ms: u32) -> Result<Option<JobResult>, String> {
        let mut r = std::mem::MaybeUninit::<sys::BfhipPoolResult>::zeroed();
        match unsafe { sys::bfhip_pool_wait(self.ptr, timeout_ms, r.as_mut_ptr()) } {
            0 => {
                let r = unsafe { r.assume_init() };
                let proof = if r.status == 0 {
                    Ok(unsafe { std::slice::from_raw_parts(r.proof_json as *const u8, r.proof_len) }.to_vec())
                } else if r.error.is_null() {
                    Err(format!("job {}: failed", r.ticket))
                } else {
                    Err(unsafe { CStr::from_ptr(r.error) }.to_string_lossy().into_owned())
                };
                unsafe {
                    sys::bfhip_free_host(r.proof_json as *mut c_void);
                    sys::bfhip_free_host(r.error as *mut c_void);
                }
                Ok(Some(JobResult { ticket: r.ticket, tag: r.user_tag, worker: r.worker, flags: r.flags, seconds_queued: r.seconds_queued,
                                    seconds_proving: r.seconds_proving, proof, cancelled: r.status == sys::BFHIP_JOB_CANCELLED }))
            }
            1 => Err("timeout".to_string()),
            2 => Ok(None),
            _ => Err(last_error()),
        }
    }

    /// `bfhip_pool_cancel`: `Ok(true)` = the job was still queued and will be delivered as cancelled.
    pub fn cancel(&self, ticket: u64) -> Result<bool, String> {
        match unsafe { sys::bfhip_pool_cancel(self.ptr, ticket) } {
            0 => Ok(true),
            1 => Ok(false),
            _ => Err(last_error()),
        }
    }

    /// `bfhip_pool_outstanding`: (queued, running, finished and not yet taken).
    pub fn outstanding(&self) -> (u32, u32, u32) {
        let (mut q, mut r, mut f) = (0u32, 0u32, 0u32);
        unsafe { sys::bfhip_pool_outstanding(self.ptr, &mut q, &mut r, &mut f) };
        (q, r, f)
    }
}

impl<'a> Drop for Pool<'a> {
    fn drop(&mut self) {
        unsafe { sys::bfhip_pool_destroy(self.ptr) };
    }
}

/// `verify_brainfuck` (`mod.rs:738-797`), host only. `Err` carries the rejection reason.
pub fn verify_brainfuck(proof_json: &[u8], log_max_rows: u32) -> Result<(), String> {
    let mut err = vec![0u8; 256];
    let rc = unsafe {
        sys::bfhip_verify_brainfuck(proof_json.as_ptr() as *const c_char, proof_json.len(), log_max_rows, err.as_mut_ptr() as *mut c_char, err.len())
    };
    match rc {
        0 => Ok(()),
        1 => Err(unsafe { CStr::from_ptr(err.as_ptr() as *const c_char) }.to_string_lossy().into_owned()),   // rejected: VerificationError name
        _ => Err(last_error()),                                                                                // internal error
    }
}

// ---- commitment-scheme session (`include/bfhip.h` "Commitment-scheme session"): commit and open ANY AIR's columns -------------------------
// stwo's `CommitmentSchemeProver` / `CommitmentSchemeVerifier` over trees of arbitrary columns, on the fused launches of a Brainfuck proof.
// An AIR that is not the snapshot's computes its traces and constraints itself and keeps everything else.

/// A secure-field element: 4 canonical M31 words. A point of the circle over it: x then y.
pub type Felt = [u32; 4];
pub type Point = [u32; 8];

fn check(rc: i32) -> Result<(), String> {
    if rc != 0 { Err(last_error()) } else { Ok(()) }
}

/// `bfhip_circle_point_offset`: `p + offset * CanonicCoset(log_size).step()` — the mask point of a column of 2^log_size rows at a row offset.
pub fn circle_point_offset(p: &Point, log_size: u32, offset: i32) -> Result<Point, String> {
    let mut out = [0u32; 8];
    check(unsafe { sys::bfhip_circle_point_offset(p.as_ptr(), log_size, offset, out.as_mut_ptr()) })?;
    Ok(out)
}

/// `Blake2sChannel::default()` / `Poseidon252Channel::default()` (by `conv.merkle_channel`): what stwo passes as `channel`. Host only.
pub struct Channel(*mut sys::BfhipChannel);

impl Channel {
    pub fn new(conv: Option<&sys::BfhipConventions>) -> Result<Self, String> {
        let mut p = std::ptr::null_mut();
        check(unsafe { sys::bfhip_channel_create(conv.map_or(std::ptr::null(), |c| c as *const _), &mut p) })?;
        Ok(Channel(p))
    }
    pub fn mix_root(&mut self, root: &[u8; 32]) -> Result<(), String> {
        check(unsafe { sys::bfhip_channel_mix_root(self.0, root.as_ptr()) })
    }
    pub fn mix_u64(&mut self, v: u64) -> Result<(), String> {
        check(unsafe { sys::bfhip_channel_mix_u64(self.0, v) })
    }
    pub fn mix_felts(&mut self, felts: &[Felt]) -> Result<(), String> {
        check(unsafe { sys::bfhip_channel_mix_felts(self.0, felts.as_ptr() as *const u32, felts.len()) })
    }
    /// stwo's `draw_felts(n)`: n = 1 is `draw_felt`, n = 2 a lookup element's (z, alpha).
    pub fn draw_felts(&mut self, n: usize) -> Result<Vec<Felt>, String> {
        let mut out = vec![[0u32; 4]; n];
        check(unsafe { sys::bfhip_channel_draw_felts(self.0, n, out.as_mut_ptr() as *mut u32) })?;
        Ok(out)
    }
    /// `CirclePoint::get_random_point`.
    pub fn draw_point(&mut self) -> Result<Point, String> {
        let mut out = [0u32; 8];
        check(unsafe { sys::bfhip_channel_draw_point(self.0, out.as_mut_ptr()) })?;
        Ok(out)
    }
    /// (digest, n_sent)
    pub fn state(&self) -> Result<([u8; 32], u32), String> {
        let (mut d, mut n) = ([0u8; 32], 0u32);
        check(unsafe { sys::bfhip_channel_state(self.0, d.as_mut_ptr(), &mut n) })?;
        Ok((d, n))
    }
    pub fn trailing_zeros(&self) -> Result<u32, String> {
        let mut n = 0u32;
        check(unsafe { sys::bfhip_channel_trailing_zeros(self.0, &mut n) })?;
        Ok(n)
    }
}

impl Drop for Channel {
    fn drop(&mut self) {
        unsafe { sys::bfhip_channel_destroy(self.0) };
    }
}

/// The sample description of `prove_values` / `verify_values`: for every column of every tree, in commit order, the indices into `points`
/// of the points it is opened at, in the order its sampled values are to appear.
pub struct Samples<'a> {
    pub points: &'a [Point],
    pub per_column: &'a [Vec<u32>],
}

impl<'a> Samples<'a> {
    fn flat(&self) -> (Vec<u32>, Vec<u32>) {
        (self.per_column.iter().map(|c| c.len() as u32).collect(), self.per_column.iter().flatten().copied().collect())
    }
}

/// `CommitmentSchemeProver` on one context (`bfhip_pcs_*`). One open session per context; while it lives the context refuses its proving,
/// checking and trace-building entries. The lifetime ties the session to its context: the context cannot be dropped first.
pub struct PcsProver<'a> {
    h: *mut sys::BfhipPcs,
    _ctx: std::marker::PhantomData<&'a Context>,
}

impl<'a> PcsProver<'a> {
    pub fn new(ctx: &'a Context) -> Result<Self, String> {
        let mut p = std::ptr::null_mut();
        check(unsafe { sys::bfhip_pcs_create(ctx.0, &mut p) })?;
        Ok(PcsProver { h: p, _ctx: std::marker::PhantomData })
    }
    /// `tree_builder.extend_evals` (`coefficients = false`) / `extend_polys` (`true`) + `commit(channel)`: device columns, column k of
    /// 2^log_sizes[k] words. Returns the root, which is mixed into `channel`.
    ///
    /// # Safety
    /// Every pointer must be a device allocation of this context's GPU holding 2^log_sizes[k] canonical words.
    pub unsafe fn commit(&mut self, channel: &mut Channel, cols: &[*const u32], log_sizes: &[u32], coefficients: bool) -> Result<[u8; 32], String> {
        assert_eq!(cols.len(), log_sizes.len());
        let mut root = [0u8; 32];
        check(sys::bfhip_pcs_commit(self.h, channel.0, cols.as_ptr(), log_sizes.as_ptr(), cols.len() as u32, coefficients as i32, root.as_mut_ptr()))?;
        Ok(root)
    }
    /// (coefficient pointers, LDE pointers) of a committed tree's columns — what the caller's constraint sweep reads; valid while `self` lives.
    pub fn tree_columns(&self, tree: u32) -> Result<(Vec<*const u32>, Vec<*const u32>), String> {
        let mut n = 0u32;
        check(unsafe { sys::bfhip_pcs_tree_columns(self.h, tree, std::ptr::null_mut(), std::ptr::null_mut(), 0, &mut n) })?;
        let (mut co, mut ev) = (vec![std::ptr::null(); n as usize], vec![std::ptr::null(); n as usize]);
        check(unsafe { sys::bfhip_pcs_tree_columns(self.h, tree, co.as_mut_ptr(), ev.as_mut_ptr(), n, &mut n) })?;
        Ok((co, ev))
    }
    /// `prove_values`: (the serde-JSON bytes of the `CommitmentSchemeProof`, the sampled values in the order of the description).
    /// Ends the session's proving life.
    pub fn prove_values(&mut self, channel: &mut Channel, samples: &Samples) -> Result<(Vec<u8>, Vec<Felt>), String> {
        let (counts, idx) = samples.flat();
        let mut sampled = vec![[0u32; 4]; idx.len()];
        let (mut js, mut len): (*mut c_char, usize) = (std::ptr::null_mut(), 0);
        check(unsafe {
            sys::bfhip_pcs_prove_values(self.h, channel.0, samples.points.as_ptr() as *const u32, samples.points.len() as u32, counts.as_ptr(), idx.as_ptr(),
                                        sampled.as_mut_ptr() as *mut u32, &mut js, &mut len)
        })?;
        let out = unsafe { std::slice::from_raw_parts(js as *const u8, len) }.to_vec();
        unsafe { sys::bfhip_free_host(js as *mut c_void) };
        Ok((out, sampled))
    }
}

impl<'a> Drop for PcsProver<'a> {
    fn drop(&mut self) {
        unsafe { sys::bfhip_pcs_destroy(self.h) };
    }
}

/// `CommitmentSchemeVerifier` (`bfhip_pcs_verifier_*`). Host only.
pub struct PcsVerifier(*mut sys::BfhipPcsVerifier);

impl PcsVerifier {
    pub fn new(conv: Option<&sys::BfhipConventions>, config: Option<&sys::BfhipPcsConfig>) -> Result<Self, String> {
        let mut p = std::ptr::null_mut();
        check(unsafe { sys::bfhip_pcs_verifier_create(conv.map_or(std::ptr::null(), |c| c as *const _), config.map_or(std::ptr::null(), |c| c as *const _), &mut p) })?;
        Ok(PcsVerifier(p))
    }
    /// `commit`: the trace-domain log sizes of the tree's columns; mixes the root into `channel`.
    pub fn commit(&mut self, channel: &mut Channel, root: &[u8; 32], log_sizes: &[u32]) -> Result<(), String> {
        check(unsafe { sys::bfhip_pcs_verifier_commit(self.0, channel.0, root.as_ptr(), log_sizes.as_ptr(), log_sizes.len() as u32) })
    }
    /// `verify_values`: `Ok(Ok(()))` accepted, `Ok(Err(name))` rejected with the `VerificationError` name, `Err` = bad arguments.
    pub fn verify_values(&mut self, channel: &mut Channel, samples: &Samples, proof_json: &[u8]) -> Result<Result<(), String>, String> {
        let (counts, idx) = samples.flat();
        let mut err = [0 as c_char; 512];
        let rc = unsafe {
            sys::bfhip_pcs_verifier_verify_values(self.0, channel.0, samples.points.as_ptr() as *const u32, samples.points.len() as u32, counts.as_ptr(), idx.as_ptr(),
                                                  proof_json.as_ptr() as *const c_char, proof_json.len(), err.as_mut_ptr(), err.len())
        };
        match rc {
            0 => Ok(Ok(())),
            1 => Ok(Err(unsafe { CStr::from_ptr(err.as_ptr()) }.to_string_lossy().into_owned())),
            _ => Err(last_error()),
        }
    }
}

impl Drop for PcsVerifier {
    fn drop(&mut self) {
        unsafe { sys::bfhip_pcs_verifier_destroy(self.0) };
    }
}

// ---- constraint programs (`include/bfhip.h` "Constraint programs"): evaluate ANY AIR's constraints ------------------------------------------
// What a `ComponentProver<HipBackend>` of an AIR the library has never seen calls: the AIR's `FrameworkEval::evaluate`, recorded once as a
// bytecode of four u32 words {op, dst, a, b} per instruction (opcodes `sys::BFHIP_AIR_*`), runs on the constraint domain in one gfx950 kernel
// and at the out-of-domain point on the host.

/// `bfhip_air_shape`.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct AirShape { pub n_cols: u32, pub n_params: u32, pub n_constraints: u32, pub n_instr: u32, pub m_regs: u32, pub q_regs: u32, pub min_offset: i32, pub max_offset: i32 }

/// A validated constraint program (`bfhip_air`). Host only to create, inspect and evaluate at a point.
pub struct AirProgram(*mut sys::BfhipAir);

impl AirProgram {
    /// `bfhip_air_create`: a refusal names the instruction index and the rule.
    pub fn new(code: &[u32], n_cols: u32, n_params: u32) -> Result<Self, String> {
        let mut p = std::ptr::null_mut();
        check(unsafe { sys::bfhip_air_create(code.as_ptr(), code.len(), n_cols, n_params, &mut p) })?;
        Ok(AirProgram(p))
    }
    pub fn shape(&self) -> Result<AirShape, String> {
        let mut o = [0u32; 8];
        check(unsafe { sys::bfhip_air_shape(self.0, o.as_mut_ptr()) })?;
        Ok(AirShape { n_cols: o[0], n_params: o[1], n_constraints: o[2], n_instr: o[3], m_regs: o[4], q_regs: o[5], min_offset: o[6] as i32, max_offset: o[7] as i32 })
    }
    /// `bfhip_air_mask`: (column, offset) by column, within a column by first use — the order of a column's samples for `PcsProver::prove_values`.
    pub fn mask(&self) -> Result<Vec<(u32, i32)>, String> {
        let mut n = 0u32;
        check(unsafe { sys::bfhip_air_mask(self.0, std::ptr::null_mut(), std::ptr::null_mut(), 0, &mut n) })?;
        let (mut cols, mut offs) = (vec![0u32; n as usize], vec![0i32; n as usize]);
        if n > 0 { check(unsafe { sys::bfhip_air_mask(self.0, cols.as_mut_ptr(), offs.as_mut_ptr(), n, &mut n) })?; }
        Ok(cols.into_iter().zip(offs).collect())
    }
    /// `bfhip_air_eval_domain`: `evaluate_constraint_quotients_on_domain` on CanonicCoset(log_size + log_expand).circle_domain(), added into `acc`.
    /// `cols`: one device column per program column (`shifts`: its storage shift, empty = all 0); `params` / `coeffs`: one QM31 per parameter / constraint.
    pub fn eval_domain(&self, ctx: &Context, log_size: u32, log_expand: u32, cols: &[*const u32], shifts: &[u32], params: &[Felt], coeffs: &[Felt], acc: &[*mut u32; 4]) -> Result<(), String> {
        if !shifts.is_empty() && shifts.len() != cols.len() { return Err("one shift per column".into()); }
        check(unsafe {
            sys::bfhip_air_eval_domain(ctx.0, self.0, log_size, log_expand, cols.as_ptr(), if shifts.is_empty() { std::ptr::null() } else { shifts.as_ptr() },
                                       params.as_ptr() as *const u32, params.len() as u32, coeffs.as_ptr() as *const u32, coeffs.len() as u32, acc.as_ptr())
        })
    }
    /// `bfhip_air_check`: stwo's `assert_constraints` on CanonicCoset(log_size) itself — per constraint, how many cells are non-zero and the
    /// lowest of them; violations are a result, not an error. `cols` / `shifts` / `params` as for `eval_domain`, at 2^(log_size - shift) cells.
    pub fn check(&self, ctx: &Context, log_size: u32, cols: &[*const u32], shifts: &[u32], params: &[Felt]) -> Result<sys::BfhipAirCheckReport, String> {
        if !shifts.is_empty() && shifts.len() != cols.len() { return Err("one shift per column".into()); }
        let mut rep = std::mem::MaybeUninit::<sys::BfhipAirCheckReport>::zeroed();
        check(unsafe {
            sys::bfhip_air_check(ctx.0, self.0, log_size, cols.as_ptr(), if shifts.is_empty() { std::ptr::null() } else { shifts.as_ptr() },
                                 params.as_ptr() as *const u32, params.len() as u32, rep.as_mut_ptr())
        })?;
        Ok(unsafe { rep.assume_init() })      // plain integers: all-zero is a value
    }
    /// `bfhip_format_air_check`: "air check: ok", or the headline and one line per failing constraint.
    pub fn format_check(report: &sys::BfhipAirCheckReport) -> Result<String, String> {
        let mut need = 0usize;
        let rc = unsafe { sys::bfhip_format_air_check(report, std::ptr::null_mut(), 0, &mut need) };
        if rc != 0 && rc != -2 { return check(rc).map(|_| String::new()); }
        let mut buf = vec![0u8; need];
        check(unsafe { sys::bfhip_format_air_check(report, buf.as_mut_ptr() as *mut std::ffi::c_char, need, std::ptr::null_mut()) })?;
        buf.pop();
        String::from_utf8(buf).map_err(|e| e.to_string())
    }
    /// `bfhip_air_eval_at_point`: stwo's PointEvaluator over the program; `mask_values` in `mask()` order.
    pub fn eval_at_point(&self, log_size: u32, point: &Point, mask_values: &[Felt], params: &[Felt], coeffs: &[Felt]) -> Result<Felt, String> {
        let mut out = [0u32; 4];
        check(unsafe {
            sys::bfhip_air_eval_at_point(self.0, log_size, point.as_ptr(), mask_values.as_ptr() as *const u32, mask_values.len() as u32, params.as_ptr() as *const u32,
                                         params.len() as u32, coeffs.as_ptr() as *const u32, coeffs.len() as u32, out.as_mut_ptr())
        })?;
        Ok(out)
    }
}

impl AirProgram {
    /// `bfhip_air_source`: the HIP source of the kernel `compile` builds (host only; the same program gives the same text).
    pub fn source(&self) -> Result<String, String> {
        let mut n = 0usize;
        check(unsafe { sys::bfhip_air_source(self.0, std::ptr::null_mut(), 0, &mut n) })?;
        let mut buf = vec![0u8; n];
        check(unsafe { sys::bfhip_air_source(self.0, buf.as_mut_ptr() as *mut std::ffi::c_char, n, &mut n) })?;
        String::from_utf8(buf).map_err(|e| e.to_string())
    }
    /// `bfhip_air_compile`: this program as its own gfx950 kernel, compiled in-process for the context's device. The kernel keeps its own
    /// copy of the program and belongs to `ctx`.
    pub fn compile(&self, ctx: &Context) -> Result<AirKernel, String> {
        let mut k = std::ptr::null_mut();
        check(unsafe { sys::bfhip_air_compile(ctx.0, self.0, &mut k) })?;
        Ok(AirKernel(k))
    }
}

impl Drop for AirProgram {
    fn drop(&mut self) {
        unsafe { sys::bfhip_air_destroy(self.0) };
    }
}

/// `bfhip_air_kernel_info`.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct AirKernelInfo { pub vgprs: u32, pub sgprs: Option<u32>, pub scratch_bytes: u32, pub lds_bytes: u32, pub code_object_bytes: u32, pub source_bytes: u32, pub compile_us: u32, pub from_cache: bool }

/// A constraint program compiled to its own kernel (`bfhip_air_kernel`): `eval_domain` is `AirProgram::eval_domain` without the interpreter —
/// the same arguments, checks, messages and result. Drop it before its context; a context destroyed first unloads the kernel.
pub struct AirKernel(*mut sys::BfhipAirKernel);

impl AirKernel {
    /// `bfhip_air_kernel_eval_domain`; `ctx` must be the context that compiled the kernel.
    pub fn eval_domain(&self, ctx: &Context, log_size: u32, log_expand: u32, cols: &[*const u32], shifts: &[u32], params: &[Felt], coeffs: &[Felt], acc: &[*mut u32; 4]) -> Result<(), String> {
        if !shifts.is_empty() && shifts.len() != cols.len() { return Err("one shift per column".into()); }
        check(unsafe {
            sys::bfhip_air_kernel_eval_domain(ctx.0, self.0, log_size, log_expand, cols.as_ptr(), if shifts.is_empty() { std::ptr::null() } else { shifts.as_ptr() },
                                              params.as_ptr() as *const u32, params.len() as u32, coeffs.as_ptr() as *const u32, coeffs.len() as u32, acc.as_ptr())
        })
    }
    pub fn info(&self) -> Result<AirKernelInfo, String> {
        let mut o = [0u32; 8];
        check(unsafe { sys::bfhip_air_kernel_info(self.0, o.as_mut_ptr()) })?;
        Ok(AirKernelInfo { vgprs: o[0], sgprs: if o[1] == u32::MAX { None } else { Some(o[1]) }, scratch_bytes: o[2], lds_bytes: o[3], code_object_bytes: o[4],
                           source_bytes: o[5], compile_us: o[6], from_cache: o[7] != 0 })
    }
}

impl Drop for AirKernel {
    fn drop(&mut self) {
        unsafe { sys::bfhip_air_kernel_destroy(self.0) };
    }
}

// ---- composition (`include/bfhip.h` "Composition"): ALL components of an AIR to the composition polynomial ----------------------------------
/// How one component of `air_compose` runs: interpreted, or as the kernel its context compiled.
pub enum AirRunner<'a> { Program(&'a AirProgram), Kernel(&'a AirKernel) }

/// One component of `air_compose`: `cols` / `shifts` / `params` as for `AirProgram::eval_domain`, on CanonicCoset(log_size + log_expand).circle_domain().
pub struct AirComponent<'a> { pub runner: AirRunner<'a>, pub log_size: u32, pub log_expand: u32, pub cols: &'a [*const u32], pub shifts: &'a [u32], pub params: &'a [Felt] }

/// One component of `air_compose_at_point`: `mask_values` in `program.mask()` order.
pub struct AirPointComponent<'a> { pub program: &'a AirProgram, pub log_size: u32, pub mask_values: &'a [Felt], pub params: &'a [Felt] }

/// `bfhip_air_compose_coeffs`: constraint g of all T = sum(n_constraints) gets random_coeff^(T - 1 - g); slice it per component for `eval_domain`.
pub fn air_compose_coeffs(n_constraints: &[u32], random_coeff: &Felt) -> Result<Vec<Felt>, String> {
    let total: usize = n_constraints.iter().filter(|&&c| c <= sys::BFHIP_AIR_MAX_CONSTRAINTS).map(|&c| c as usize).sum();
    let mut out = vec![[0u32; 4]; total.max(1)];
    check(unsafe { sys::bfhip_air_compose_coeffs(n_constraints.as_ptr(), n_constraints.len() as u32, random_coeff.as_ptr(), out.as_mut_ptr() as *mut u32) })?;
    out.truncate(total);
    Ok(out)
}

/// `bfhip_air_compose`: `ComponentProvers::compute_composition_polynomial` — the 4 coefficient columns of 2^dst_log words into `dst`
/// (overwritten), ready for `PcsProver::commit` (form 1). `dst_log` = the largest log_size + log_expand of the list. Interpreted components
/// run in one launch, compiled ones in one launch each behind it; works while a session is open.
pub fn air_compose(ctx: &Context, comps: &[AirComponent], random_coeff: &Felt, dst_log: u32, dst: &[*mut u32; 4]) -> Result<(), String> {
    let mut raw = Vec::with_capacity(comps.len());
    for c in comps {
        if !c.shifts.is_empty() && c.shifts.len() != c.cols.len() { return Err("one shift per column".into()); }
        let (program, kernel) = match c.runner { AirRunner::Program(p) => (p.0 as *const sys::BfhipAir, std::ptr::null_mut()), AirRunner::Kernel(k) => (std::ptr::null(), k.0) };
        raw.push(sys::BfhipAirComponent { program, kernel, log_size: c.log_size, log_expand: c.log_expand, cols_h: c.cols.as_ptr(),
                                          col_shifts_h: if c.shifts.is_empty() { std::ptr::null() } else { c.shifts.as_ptr() },
                                          params_h: c.params.as_ptr() as *const u32, n_params: c.params.len() as u32, reserved: 0 });
    }
    check(unsafe { sys::bfhip_air_compose(ctx.0, raw.as_ptr(), raw.len() as u32, random_coeff.as_ptr(), dst_log, dst.as_ptr()) })
}

/// `bfhip_air_compose_at_point` (host only): `Components::eval_composition_polynomial_at_point` from the sampled mask values.
pub fn air_compose_at_point(comps: &[AirPointComponent], point: &Point, random_coeff: &Felt) -> Result<Felt, String> {
    let raw: Vec<sys::BfhipAirPointComponent> = comps.iter().map(|c| sys::BfhipAirPointComponent {
        program: c.program.0 as *const sys::BfhipAir, log_size: c.log_size, n_mask: c.mask_values.len() as u32, mask_values_h: c.mask_values.as_ptr() as *const u32,
        params_h: c.params.as_ptr() as *const u32, n_params: c.params.len() as u32, reserved: 0 }).collect();
    let mut out = [0u32; 4];
    check(unsafe { sys::bfhip_air_compose_at_point(raw.as_ptr(), raw.len() as u32, point.as_ptr(), random_coeff.as_ptr(), out.as_mut_ptr()) })?;
    Ok(out)
}

/// One component of `logup_program_generate_batch`: `cols` / `shifts` / `params` / `out` as for `LogupProgram::generate`.
pub struct LogupComponent<'a> { pub program: &'a LogupProgram, pub log_size: u32, pub cols: &'a [*const u32], pub shifts: &'a [u32], pub params: &'a [Felt], pub out: &'a [*mut u32] }

/// `bfhip_logup_program_generate_batch`: the interaction trace of ALL components in one call (one allocation, the row stage in one launch for
/// the components below 2^16 cells and one per larger one, three scan launches, one read-back). Returns every component's claimed sum, word
/// for word `LogupProgram::generate`'s, and their sum. No output column may overlap another column of the list; works while a session is
/// open. A zero denominator is an `Err` that names the lowest such component, the fraction and the cell.
pub fn logup_program_generate_batch(ctx: &Context, comps: &[LogupComponent]) -> Result<(Vec<Felt>, Felt), String> {
    let mut raw = Vec::with_capacity(comps.len());
    for c in comps {
        if !c.shifts.is_empty() && c.shifts.len() != c.cols.len() { return Err("one shift per column".into()); }
        if c.out.len() != 4 * c.program.shape()?.n_logup_cols as usize { return Err("4 coordinate columns per logUp column".into()); }
        raw.push(sys::BfhipLogupComponent { program: c.program.0 as *const sys::BfhipLogup, log_size: c.log_size, n_params: c.params.len() as u32, cols_h: c.cols.as_ptr(),
                                            col_shifts_h: if c.shifts.is_empty() { std::ptr::null() } else { c.shifts.as_ptr() },
                                            params_h: c.params.as_ptr() as *const u32, out_cols_h: c.out.as_ptr(), reserved: 0 });
    }
    let (mut claimed, mut total) = (vec![[0u32; 4]; comps.len().max(1)], [0u32; 4]);
    check(unsafe { sys::bfhip_logup_program_generate_batch(ctx.0, raw.as_ptr(), raw.len() as u32, claimed.as_mut_ptr() as *mut u32, total.as_mut_ptr()) })?;
    claimed.truncate(comps.len());
    Ok((claimed, total))
}

// ---- row order <-> storage order (`include/bfhip.h` "Row order") --------------------------------------------------------------------------------
/// A device table in row order: row-major (`word (r, c)` at `rows[r * row_stride + c]`, `row_stride >= n_cols` words) or one device
/// pointer per source column.
pub enum RowsTable<'a> {
    RowMajor { rows: *const u32, n_rows: u64, n_cols: u32, row_stride: u64 },
    ColumnMajor { cols: &'a [*const u32], n_rows: u64 },
}

/// `bfhip_columns_from_rows`: a trace in ROW order (row r + 1 = the row at offset +1) to storage-order columns of `2^log_size` words, one
/// launch. `src_cols` empty = the identity; otherwise the source column of every output column (subset, permutation, repeats). Rows from
/// `n_rows` on hold `pad[k]` (`pad` empty = 0), or with `repeat_last` a copy of the last row. Every word read is checked: a non-canonical
/// one is an `Err` naming the lowest row, then the lowest output column. Takes nothing from the arena; works while a session is open.
pub fn columns_from_rows(ctx: &Context, table: &RowsTable, log_size: u32, src_cols: &[u32], pad: &[u32], repeat_last: bool, out: &[*mut u32]) -> Result<(), String> {
    if !src_cols.is_empty() && src_cols.len() != out.len() { return Err("one source column per output column".into()); }
    if !pad.is_empty() && pad.len() != out.len() { return Err("one pad value per output column".into()); }
    let flags = if repeat_last { sys::BFHIP_ROWS_REPEAT_LAST } else { 0 };
    let raw = match *table {
        RowsTable::RowMajor { rows, n_rows, n_cols, row_stride } =>
            sys::BfhipRowsTable { layout: sys::BFHIP_ROWS_ROW_MAJOR, n_cols, rows_d: rows, cols_h: std::ptr::null(), n_rows, row_stride, flags, reserved: 0 },
        RowsTable::ColumnMajor { cols, n_rows } =>
            sys::BfhipRowsTable { layout: sys::BFHIP_ROWS_COLUMN_MAJOR, n_cols: cols.len() as u32, rows_d: std::ptr::null(), cols_h: cols.as_ptr(), n_rows, row_stride: 0, flags, reserved: 0 },
    };
    check(unsafe { sys::bfhip_columns_from_rows(ctx.0, &raw, log_size, if src_cols.is_empty() { std::ptr::null() } else { src_cols.as_ptr() },
                                                if pad.is_empty() { std::ptr::null() } else { pad.as_ptr() }, out.as_ptr(), out.len() as u32) })
}

fn raw_rows_table(table: &RowsTable, flags: u32) -> sys::BfhipRowsTable {
    match *table {
        RowsTable::RowMajor { rows, n_rows, n_cols, row_stride } =>
            sys::BfhipRowsTable { layout: sys::BFHIP_ROWS_ROW_MAJOR, n_cols, rows_d: rows, cols_h: std::ptr::null(), n_rows, row_stride, flags, reserved: 0 },
        RowsTable::ColumnMajor { cols, n_rows } =>
            sys::BfhipRowsTable { layout: sys::BFHIP_ROWS_COLUMN_MAJOR, n_cols: cols.len() as u32, rows_d: std::ptr::null(), cols_h: cols.as_ptr(), n_rows, row_stride: 0, flags, reserved: 0 },
    }
}

/// `bfhip_rows_select` (`include/bfhip.h` "Row selection"): `columns_from_rows` of a selection of the table's rows. A candidate row
/// `rows.0 .. rows.1` is selected iff every term holds (`word(row, col) <op> value` as integers, `op` = `sys::BFHIP_SELECT_EQ` ..
/// `BFHIP_SELECT_GE`); the selected rows are sorted by `keys`, most significant first, stably; output row `i` of output column `k` is the
/// source word `(order[i] + outs[k].offset, outs[k].col)`, rows past the selected ones hold `outs[k].pad`, or with `repeat_last` the last
/// selected row. `out` empty with `log_size` 0 is the count-only form. `order`: null, or `rows.1 - rows.0` device words for the source row
/// of every selected row. Returns the number of selected rows. Takes nothing from the arena; works while a session is open.
/// Source only, like the rest of this file: it has never been compiled.
pub fn rows_select(ctx: &Context, table: &RowsTable, terms: &[sys::BfhipSelectTerm], keys: &[sys::BfhipSelectKey], rows: (u64, u64), log_size: u32,
                   outs: &[sys::BfhipSelectOut], repeat_last: bool, out: &[*mut u32], order: *mut u32) -> Result<u64, String> {
    if outs.len() != out.len() { return Err("one output pointer per output column".into()); }
    let raw = raw_rows_table(table, if repeat_last { sys::BFHIP_ROWS_REPEAT_LAST } else { 0 });
    let sel = sys::BfhipRowsSelectDesc { terms: if terms.is_empty() { std::ptr::null() } else { terms.as_ptr() }, keys: if keys.is_empty() { std::ptr::null() } else { keys.as_ptr() },
                                         n_terms: terms.len() as u32, n_keys: keys.len() as u32, row_begin: rows.0, row_end: rows.1, reserved: [0; 2] };
    let mut n_selected = 0u64;
    check(unsafe { sys::bfhip_rows_select(ctx.0, &raw, &sel, log_size, if outs.is_empty() { std::ptr::null() } else { outs.as_ptr() },
                                          if out.is_empty() { std::ptr::null() } else { out.as_ptr() }, out.len() as u32, order, &mut n_selected) })?;
    Ok(n_selected)
}

/// `bfhip_rows_fill` (`include/bfhip.h` "Row filling"): the entries of the table — source rows `order[0 .. n_entries]` (device words, as
/// `rows_select` writes them), or with a null `order` the rows `row_begin .. row_begin + n_entries` — with the missing rows inserted. With
/// `gaps` a row for every value of `step` (a source column) skipped between two consecutive entries that agree in every `group` column;
/// behind the last entry inserted rows without end. Output row `i` of output column `k` is sequence element `i + outs[k].offset`; its value
/// follows `outs[k].kind` (`sys::BFHIP_FILL_KEEP`, `SET`, `MARK`). `out` empty with `log_size` 0 is the count-only form. Returns the number
/// of rows before the tail. Takes nothing from the arena; works while a session is open.
/// Source only, like the rest of this file: it has never been compiled.
pub fn rows_fill(ctx: &Context, table: &RowsTable, group: &[u32], step: Option<u32>, gaps: bool, order: *const u32, n_entries: u64, row_begin: u64, log_size: u32,
                 outs: &[sys::BfhipFillOut], out: &[*mut u32]) -> Result<u64, String> {
    if outs.len() != out.len() { return Err("one output pointer per output column".into()); }
    let raw = raw_rows_table(table, 0);
    let fill = sys::BfhipRowsFillDesc { group_cols: if group.is_empty() { std::ptr::null() } else { group.as_ptr() }, n_group: group.len() as u32,
                                        step_col: step.unwrap_or(sys::BFHIP_FILL_NO_STEP), order_d: order, n_entries, row_begin,
                                        flags: if gaps { sys::BFHIP_FILL_GAPS } else { 0 }, reserved: 0 };
    let mut n_filled = 0u64;
    check(unsafe { sys::bfhip_rows_fill(ctx.0, &raw, &fill, log_size, if outs.is_empty() { std::ptr::null() } else { outs.as_ptr() },
                                        if out.is_empty() { std::ptr::null() } else { out.as_ptr() }, out.len() as u32, &mut n_filled) })?;
    Ok(n_filled)
}

/// `bfhip_rows_from_columns`: the inverse — storage-order columns to words `(r, c)`, `r < n_rows`, `c < cols.len()`, of a row-major device
/// table; the rest of each row is left untouched. Enqueued on the context's stream; no canonicity check.
pub fn rows_from_columns(ctx: &Context, cols: &[*const u32], log_size: u32, rows: *mut u32, n_rows: u64, row_stride: u64) -> Result<(), String> {
    check(unsafe { sys::bfhip_rows_from_columns(ctx.0, cols.as_ptr(), cols.len() as u32, log_size, rows, n_rows, row_stride, 0) })
}

/// `bfhip_cell_of_row` (host only): the storage index of coset index `row`.
pub fn cell_of_row(log_size: u32, row: u64) -> Result<u64, String> {
    let mut cell = 0u64;
    check(unsafe { sys::bfhip_cell_of_row(log_size, row, &mut cell) })?;
    Ok(cell)
}

/// `bfhip_row_of_cell` (host only): the row an author wrote for the cell that `AirProgram::check` or a logUp generation reports.
pub fn row_of_cell(log_size: u32, cell: u64) -> Result<u64, String> {
    let mut row = 0u64;
    check(unsafe { sys::bfhip_row_of_cell(log_size, cell, &mut row) })?;
    Ok(row)
}

// ---- the protocol driver (`include/bfhip.h` "Proving an AIR given as programs") ----------------------------------------------------------------
// `prover::prove` / `verify` for an AIR given as a statement: trees, relations, components with their column bindings and parameter rules.
// `air_prove` orders the session, the mixes and draws, the batched interaction trace, `air_compose`, the mask and `prove_values`;
// `air_verify` replays it on the host. The statement holds no device pointers and is shared by both.

/// A caller tree of an `AirStatement`: trace-domain log sizes, form (0 = evaluations, 1 = coefficients) and the words mixed in front of its commit.
pub struct AirStatementTree { pub log_sizes: Vec<u32>, pub form: u32, pub mix_u64: Vec<u64> }

/// `columns[c]` = (tree, column) for column c of `program`; tree `sys::BFHIP_AIR_TREE_INTERACTION` = the component's own j-th interaction
/// coordinate column. `fraction_columns` likewise for `fractions`. `params`: one rule per parameter of `program` (`AirStatement::z` ...).
pub struct AirStatementComponent<'a> {
    pub program: &'a AirProgram, pub fractions: Option<&'a LogupProgram>, pub log_size: u32, pub log_expand: u32,
    pub columns: Vec<(u32, u32)>, pub fraction_columns: Vec<(u32, u32)>, pub params: Vec<sys::BfhipAirParamRule>,
}

/// `bfhip_air_statement`, owned: build it with `tree` and `component`, pass it to `air_prove` and `air_verify`.
pub struct AirStatement<'a> { pub n_relations: u32, pub trees: Vec<AirStatementTree>, pub components: Vec<AirStatementComponent<'a>> }

// what a `sys::BfhipAirStatement` points into, alive for one call
struct RawStatement { _cols: Vec<[Vec<u32>; 4]>, _trees: Vec<sys::BfhipAirStatementTree>, _comps: Vec<sys::BfhipAirStatementComponent>, st: sys::BfhipAirStatement }

impl<'a> AirStatement<'a> {
    pub fn new(n_relations: u32) -> Self { AirStatement { n_relations, trees: Vec::new(), components: Vec::new() } }
    pub fn const_param(value: Felt) -> sys::BfhipAirParamRule { sys::BfhipAirParamRule { kind: sys::BFHIP_AIR_PARAM_CONST, relation: 0, power: 0, reserved: 0, value } }
    pub fn z(relation: u32) -> sys::BfhipAirParamRule { sys::BfhipAirParamRule { kind: sys::BFHIP_AIR_PARAM_LOOKUP_Z, relation, power: 0, reserved: 0, value: [0; 4] } }
    pub fn alpha_pow(relation: u32, power: u32) -> sys::BfhipAirParamRule { sys::BfhipAirParamRule { kind: sys::BFHIP_AIR_PARAM_LOOKUP_ALPHA_POW, relation, power, reserved: 0, value: [0; 4] } }
    pub fn claimed_sum() -> sys::BfhipAirParamRule { sys::BfhipAirParamRule { kind: sys::BFHIP_AIR_PARAM_CLAIMED_SUM, relation: 0, power: 0, reserved: 0, value: [0; 4] } }
    /// A caller tree; returns its index.
    pub fn tree(&mut self, log_sizes: &[u32], form: u32, mix_u64: &[u64]) -> u32 {
        self.trees.push(AirStatementTree { log_sizes: log_sizes.to_vec(), form, mix_u64: mix_u64.to_vec() });
        self.trees.len() as u32 - 1
    }
    /// A component; returns its index.
    pub fn component(&mut self, component: AirStatementComponent<'a>) -> u32 {
        self.components.push(component);
        self.components.len() as u32 - 1
    }
    fn raw(&self) -> RawStatement {
        let cols: Vec<[Vec<u32>; 4]> = self.components.iter().map(|c| [c.columns.iter().map(|p| p.0).collect(), c.columns.iter().map(|p| p.1).collect(),
                                                                       c.fraction_columns.iter().map(|p| p.0).collect(), c.fraction_columns.iter().map(|p| p.1).collect()]).collect();
        let trees: Vec<sys::BfhipAirStatementTree> = self.trees.iter().map(|t| sys::BfhipAirStatementTree {
            n_cols: t.log_sizes.len() as u32, form: t.form, log_sizes_h: t.log_sizes.as_ptr(), mix_u64_h: t.mix_u64.as_ptr(), n_mix: t.mix_u64.len() as u32, reserved: 0 }).collect();
        let comps: Vec<sys::BfhipAirStatementComponent> = self.components.iter().zip(cols.iter()).map(|(c, a)| sys::BfhipAirStatementComponent {
            program: c.program.0 as *const sys::BfhipAir, fractions: c.fractions.map_or(std::ptr::null(), |f| f.0 as *const sys::BfhipLogup), log_size: c.log_size,
            log_expand: c.log_expand, col_trees_h: a[0].as_ptr(), col_columns_h: a[1].as_ptr(), frac_trees_h: a[2].as_ptr(), frac_columns_h: a[3].as_ptr(),
            params_h: c.params.as_ptr(), n_params: c.params.len() as u32, reserved: 0 }).collect();
        let st = sys::BfhipAirStatement { trees: trees.as_ptr(), components: comps.as_ptr(), n_trees: trees.len() as u32, n_relations: self.n_relations,
                                          n_components: comps.len() as u32, reserved: 0 };
        RawStatement { _cols: cols, _trees: trees, _comps: comps, st }      // moving a Vec does not move its heap block: the pointers hold
    }
}

/// `bfhip_air_prove`: the whole proof of the statement's AIR. `tree_cols[t][c]` = device column c of caller tree t (full size); `kernels`:
/// empty, or per component `None` / the `AirKernel` this context compiled of its program; `check`: `BFHIP_AIR_PROVE_CHECK`. Returns the bytes
/// `{"claimed_sums": [...], "proof": <CommitmentSchemeProof>}` that `air_verify` takes. No session is left open, whatever the outcome.
pub fn air_prove(ctx: &Context, statement: &AirStatement, tree_cols: &[&[*const u32]], kernels: &[Option<&AirKernel>], channel: &mut Channel, check_trace: bool) -> Result<Vec<u8>, String> {
    if tree_cols.len() != statement.trees.len() || tree_cols.iter().zip(statement.trees.iter()).any(|(c, t)| c.len() != t.log_sizes.len()) {
        return Err("one device column per column of every caller tree".into());
    }
    if !kernels.is_empty() && kernels.len() != statement.components.len() { return Err("one kernel (or None) per component".into()); }
    let raw = statement.raw();
    let trees: Vec<*const *const u32> = tree_cols.iter().map(|c| c.as_ptr()).collect();
    let ks: Vec<*mut sys::BfhipAirKernel> = kernels.iter().map(|k| k.map_or(std::ptr::null_mut(), |k| k.0)).collect();
    let (mut js, mut len): (*mut c_char, usize) = (std::ptr::null_mut(), 0);
    check(unsafe {
        sys::bfhip_air_prove(ctx.0, &raw.st, trees.as_ptr(), if ks.is_empty() { std::ptr::null() } else { ks.as_ptr() }, channel.0,
                             if check_trace { sys::BFHIP_AIR_PROVE_CHECK } else { 0 }, &mut js, &mut len)
    })?;
    let out = unsafe { std::slice::from_raw_parts(js as *const u8, len) }.to_vec();
    unsafe { sys::bfhip_free_host(js as *mut c_void) };
    Ok(out)
}

/// `bfhip_air_verify` (host only): `Ok(Ok(()))` accepted, `Ok(Err(name))` rejected with the `VerificationError` name, `Err` = a statement the
/// validator refuses or bad arguments. `channel`: a fresh channel carrying what the prover's carried before `air_prove`.
pub fn air_verify(statement: &AirStatement, conv: Option<&sys::BfhipConventions>, config: Option<&sys::BfhipPcsConfig>, channel: &mut Channel, proof_json: &[u8]) -> Result<Result<(), String>, String> {
    let raw = statement.raw();
    let mut err = [0 as c_char; 512];
    let rc = unsafe {
        sys::bfhip_air_verify(&raw.st, conv.map_or(std::ptr::null(), |c| c as *const _), config.map_or(std::ptr::null(), |c| c as *const _), channel.0,
                              proof_json.as_ptr() as *const c_char, proof_json.len(), err.as_mut_ptr(), err.len())
    };
    match rc {
        0 => Ok(Ok(())),
        1 => Ok(Err(unsafe { CStr::from_ptr(err.as_ptr()) }.to_string_lossy().into_owned())),
        _ => Err(last_error()),
    }
}

// ---- fraction programs (`include/bfhip.h` "Fraction programs"): the logUp interaction trace of ANY AIR ---------------------------------------
// What a component's `interaction_trace_evaluation` hands to `LogupTraceGenerator::{new_col, write_frac, finalize_col, finalize_last}`, recorded
// once as bytecode: a constraint program's opcodes without constraints, plus `sys::BFHIP_LOGUP_FRAC` {-, a, b} (add q[a] / q[b] to the open
// column) and `sys::BFHIP_LOGUP_END_COL`. It runs on the trace domain over columns whose cells are all distinct.

/// `bfhip_logup_shape`.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct LogupShape { pub n_cols: u32, pub n_params: u32, pub n_logup_cols: u32, pub n_fractions: u32, pub n_instr: u32, pub m_regs: u32, pub q_regs: u32 }

/// A validated fraction program (`bfhip_logup`). Host only to create and inspect.
pub struct LogupProgram(*mut sys::BfhipLogup);

impl LogupProgram {
    /// `bfhip_logup_create`: a refusal names the instruction index and the rule.
    pub fn new(code: &[u32], n_cols: u32, n_params: u32) -> Result<Self, String> {
        let mut p = std::ptr::null_mut();
        check(unsafe { sys::bfhip_logup_create(code.as_ptr(), code.len(), n_cols, n_params, &mut p) })?;
        Ok(LogupProgram(p))
    }
    pub fn shape(&self) -> Result<LogupShape, String> {
        let mut o = [0u32; 8];
        check(unsafe { sys::bfhip_logup_shape(self.0, o.as_mut_ptr()) })?;
        Ok(LogupShape { n_cols: o[0], n_params: o[1], n_logup_cols: o[2], n_fractions: o[3], n_instr: o[4], m_regs: o[5], q_regs: o[6] })
    }
    /// `bfhip_logup_program_generate`: the interaction trace on CanonicCoset(log_size).circle_domain(); returns the claimed sum. `cols`: one device
    /// column per program column (`shifts`: its storage shift, empty = all 0); `out`: 4 full-size coordinate columns per logUp column. A zero
    /// denominator is an `Err` that names the fraction and the cell.
    pub fn generate(&self, ctx: &Context, log_size: u32, cols: &[*const u32], shifts: &[u32], params: &[Felt], out: &[*mut u32]) -> Result<Felt, String> {
        if !shifts.is_empty() && shifts.len() != cols.len() { return Err("one shift per column".into()); }
        if out.len() != 4 * self.shape()?.n_logup_cols as usize { return Err("4 coordinate columns per logUp column".into()); }
        let mut claimed = [0u32; 4];
        check(unsafe {
            sys::bfhip_logup_program_generate(ctx.0, self.0, log_size, cols.as_ptr(), if shifts.is_empty() { std::ptr::null() } else { shifts.as_ptr() },
                                              params.as_ptr() as *const u32, params.len() as u32, out.as_ptr(), claimed.as_mut_ptr())
        })?;
        Ok(claimed)
    }
}

impl Drop for LogupProgram {
    fn drop(&mut self) {
        unsafe { sys::bfhip_logup_destroy(self.0) };
    }
}

// ---- relation programs (`include/bfhip.h` "Relation programs"): the lookup tuples of ANY AIR that do not cancel --------------------------------
// A component's `add_to_relation(relation, multiplicity, values)` calls, recorded once as bytecode: the base-field opcodes of a constraint
// program, plus `sys::BFHIP_REL_WORD` {-, a} (append m[a] to the pending tuple) and `sys::BFHIP_REL_ENTRY` {relation, a} (the entry, with
// multiplicity m[a]). stwo's relation tracker for an AIR the library has never seen: run it in front of the session, it needs no lookup
// elements.

/// `bfhip_relation_program_shape`.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct RelationShape { pub n_cols: u32, pub n_relations: u32, pub n_entries: u32, pub n_instr: u32, pub m_regs: u32 }

/// One table of `RelationProgram::summary`: a program over a component's columns. `cols`: one device column per program column; the program
/// is evaluated once per 2^row_shift cells; `shifts`: column k holds 2^(log_size - shifts[k]) words (empty = every column holds one word per
/// evaluated row).
pub struct RelationProgramTable<'a> { pub program: &'a RelationProgram, pub log_size: u32, pub row_shift: u32, pub cols: &'a [*const u32], pub shifts: &'a [u32] }

/// A validated relation program (`bfhip_relation_program`). Host only to create, inspect and evaluate on one row.
pub struct RelationProgram(*mut sys::BfhipRelationProgram);

impl RelationProgram {
    /// `bfhip_relation_program_create`: `relation_words[r]` = the width of relation r (1 to 7). A refusal names the instruction index and the rule.
    pub fn new(code: &[u32], n_cols: u32, relation_words: &[u32]) -> Result<Self, String> {
        let mut p = std::ptr::null_mut();
        let widths: Vec<u32> = if relation_words.is_empty() { vec![0] } else { relation_words.to_vec() };
        check(unsafe { sys::bfhip_relation_program_create(code.as_ptr(), code.len(), n_cols, widths.as_ptr(), relation_words.len() as u32, &mut p) })?;
        Ok(RelationProgram(p))
    }
    pub fn shape(&self) -> Result<RelationShape, String> {
        let mut o = [0u32; 8];
        check(unsafe { sys::bfhip_relation_program_shape(self.0, o.as_mut_ptr()) })?;
        Ok(RelationShape { n_cols: o[0], n_relations: o[1], n_entries: o[2], n_instr: o[3], m_regs: o[4] })
    }
    /// `bfhip_relation_program_eval_row` (host only): the entries of one row in program order, zero multiplicities included, as
    /// (relation, multiplicity, the tuple zero padded to 7 words).
    pub fn eval_row(&self, col_values: &[u32]) -> Result<Vec<(u32, u32, [u32; 7])>, String> {
        let n_entries = self.shape()?.n_entries as usize;
        if col_values.len() != self.shape()?.n_cols as usize { return Err("one value per program column".into()); }
        let (mut rel, mut mult, mut tup, mut n) = (vec![0u32; n_entries], vec![0u32; n_entries], vec![0u32; 7 * n_entries], 0u32);
        check(unsafe { sys::bfhip_relation_program_eval_row(self.0, col_values.as_ptr(), rel.as_mut_ptr(), mult.as_mut_ptr(), tup.as_mut_ptr(), n_entries as u32, &mut n) })?;
        Ok((0..n as usize).map(|e| { let mut t = [0u32; 7]; t.copy_from_slice(&tup[7 * e..7 * e + 7]); (rel[e], mult[e], t) }).collect())
    }
    /// `bfhip_relation_program_summary` over 1..64 tables whose programs share one list of relations: per relation its counts and up to
    /// `max_entries` tuples whose multiplicities do not cancel, in lexicographic order. An imbalance is a result, not an `Err`. Refused while a
    /// commitment-scheme session is open on the context.
    pub fn summary(ctx: &Context, tables: &[RelationProgramTable], max_entries: u32) -> Result<(Vec<sys::BfhipRelationReport>, Vec<sys::BfhipRelationEntry>), String> {
        let first = tables.first().ok_or("1 to 64 tables")?;
        let n_rel = first.program.shape()?.n_relations as usize;
        for t in tables {
            if t.cols.len() != t.program.shape()?.n_cols as usize || (!t.shifts.is_empty() && t.shifts.len() != t.cols.len()) { return Err("one column pointer (and shift) per program column".into()); }
        }
        let raw: Vec<sys::BfhipRelationProgramTable> = tables.iter().map(|t| sys::BfhipRelationProgramTable {
            program: t.program.0, log_size: t.log_size, row_shift: t.row_shift, cols_h: t.cols.as_ptr(),
            col_shifts_h: if t.shifts.is_empty() { std::ptr::null() } else { t.shifts.as_ptr() } }).collect();
        let mut reports = vec![sys::BfhipRelationReport::default(); n_rel];
        let mut entries = vec![sys::BfhipRelationEntry::default(); n_rel * max_entries as usize];
        let entries_ptr = if max_entries == 0 { std::ptr::null_mut() } else { entries.as_mut_ptr() };
        check(unsafe { sys::bfhip_relation_program_summary(ctx.0, raw.as_ptr(), raw.len() as u32, n_rel as u32, reports.as_mut_ptr(), entries_ptr, max_entries) })?;
        let mut listed = Vec::new();
        for (r, rep) in reports.iter().enumerate() {
            listed.extend_from_slice(&entries[r * max_entries as usize..r * max_entries as usize + rep.n_reported as usize]);
        }
        Ok((reports, listed))
    }
    /// `bfhip_relation_program_multiplicities`: fills `out` — one word per evaluated row of `tables[target_table]`, a device pointer, which
    /// may be the column the target's multiplicity operand reads — with the net of every other entry of `relation` at the lowest row holding
    /// each tuple, and returns the counts and up to `max_missing` tuples with a non-zero net that no row of the target holds. The target is
    /// the `target_entry`-th ENTRY of `relation` in that table's program. Missing tuples are a result, not an `Err`. Refused while a
    /// commitment-scheme session is open on the context.
    pub fn multiplicities(ctx: &Context, tables: &[RelationProgramTable], relation: u32, target_table: u32, target_entry: u32, out: *mut u32,
                          max_missing: u32) -> Result<(sys::BfhipMultiplicityReport, Vec<sys::BfhipRelationEntry>), String> {
        let first = tables.first().ok_or("1 to 64 tables")?;
        let n_rel = first.program.shape()?.n_relations;
        for t in tables {
            if t.cols.len() != t.program.shape()?.n_cols as usize || (!t.shifts.is_empty() && t.shifts.len() != t.cols.len()) { return Err("one column pointer (and shift) per program column".into()); }
        }
        let raw: Vec<sys::BfhipRelationProgramTable> = tables.iter().map(|t| sys::BfhipRelationProgramTable {
            program: t.program.0, log_size: t.log_size, row_shift: t.row_shift, cols_h: t.cols.as_ptr(),
            col_shifts_h: if t.shifts.is_empty() { std::ptr::null() } else { t.shifts.as_ptr() } }).collect();
        let mut report = sys::BfhipMultiplicityReport::default();
        let mut missing = vec![sys::BfhipRelationEntry::default(); max_missing as usize];
        let missing_ptr = if max_missing == 0 { std::ptr::null_mut() } else { missing.as_mut_ptr() };
        check(unsafe { sys::bfhip_relation_program_multiplicities(ctx.0, raw.as_ptr(), raw.len() as u32, n_rel, relation, target_table, target_entry, out, &mut report, missing_ptr, max_missing) })?;
        missing.truncate(report.n_reported as usize);
        Ok((report, missing))
    }
}

impl Drop for RelationProgram {
    fn drop(&mut self) {
        unsafe { sys::bfhip_relation_program_destroy(self.0) };
    }
}

// ---- witness programs (`include/bfhip.h` "Witness programs"): the columns an author computes row by row, derived on the device ----------------
// The base-field opcodes of a constraint program, M_COL at trace offsets, plus `sys::BFHIP_WIT_ARG` .. `sys::BFHIP_WIT_STORE`: run once per
// row of CanonicCoset(log_size), a program reads input columns and stores output columns — an inverse, a padding flag, the bits of a byte, a
// "next" value. The step between `Context::columns_from_rows` and the first commitment.

/// `bfhip_witness_program_shape`.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct WitnessShape { pub n_cols: u32, pub n_out: u32, pub n_args: u32, pub n_instr: u32, pub m_regs: u32, pub min_offset: i32, pub max_offset: i32 }

/// A validated witness program (`bfhip_witness_program`). Host only to create, inspect and evaluate over a row-order table.
pub struct WitnessProgram(*mut sys::BfhipWitnessProgram);

impl WitnessProgram {
    /// `bfhip_witness_program_create`. A refusal names the instruction index and the rule.
    pub fn new(code: &[u32], n_cols: u32, n_out: u32, n_args: u32) -> Result<Self, String> {
        let mut p = std::ptr::null_mut();
        check(unsafe { sys::bfhip_witness_program_create(code.as_ptr(), code.len(), n_cols, n_out, n_args, &mut p) })?;
        Ok(WitnessProgram(p))
    }
    pub fn shape(&self) -> Result<WitnessShape, String> {
        let mut o = [0u32; 8];
        check(unsafe { sys::bfhip_witness_program_shape(self.0, o.as_mut_ptr()) })?;
        Ok(WitnessShape { n_cols: o[0], n_out: o[1], n_args: o[2], n_instr: o[3], m_regs: o[4], min_offset: o[5] as i32, max_offset: o[6] as i32 })
    }
    /// `bfhip_witness_program_eval_table` (host only): the program over a row-major table of 2^log_size rows in ROW order; returns the
    /// 2^log_size x n_out outputs, row-major. The definition `generate` is held to.
    pub fn eval_table(&self, log_size: u32, table: &[u32], args: &[u32]) -> Result<Vec<u32>, String> {
        let s = self.shape()?;
        if log_size < 1 || log_size > 30 || table.len() != (s.n_cols as usize) << log_size { return Err("a table is 2^log_size x n_cols words".into()); }
        let mut out = vec![0u32; (s.n_out as usize) << log_size];
        let table_ptr = if table.is_empty() { std::ptr::null() } else { table.as_ptr() };
        let args_ptr = if args.is_empty() { std::ptr::null() } else { args.as_ptr() };
        check(unsafe { sys::bfhip_witness_program_eval_table(self.0, log_size, table_ptr, args_ptr, args.len() as u32, out.as_mut_ptr()) })?;
        Ok(out)
    }
    /// `bfhip_witness_program_generate`: the program at every cell of the trace domain, one launch on the context's stream, no read-back.
    /// `cols` and `out_cols`: device columns of 2^log_size words in storage order. Works while a commitment-scheme session is open.
    pub fn generate(&self, ctx: &Context, log_size: u32, cols: &[*const u32], args: &[u32], out_cols: &[*mut u32]) -> Result<(), String> {
        if cols.len() != self.shape()?.n_cols as usize { return Err("one column pointer per program column".into()); }
        let cols_ptr = if cols.is_empty() { std::ptr::null() } else { cols.as_ptr() };
        let args_ptr = if args.is_empty() { std::ptr::null() } else { args.as_ptr() };
        check(unsafe { sys::bfhip_witness_program_generate(ctx.0, self.0, log_size, cols_ptr, args_ptr, args.len() as u32, out_cols.as_ptr(), out_cols.len() as u32) })
    }
}

impl Drop for WitnessProgram {
    fn drop(&mut self) {
        unsafe { sys::bfhip_witness_program_destroy(self.0) };
    }
}
