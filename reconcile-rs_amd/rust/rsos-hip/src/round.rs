//! One `rbsr` protocol round answered inside the library (`rh_store_protocol_round` /
//! `rh_sstore_protocol_round`, include/rsos_hip.h): `protocol_round_with_policy`
//! (rbsr/src/protocol.rs:212-317) for the policies that decide on the span alone, and
//! `rh_store_protocol_round_threshold` / `rh_sstore_protocol_round_threshold` for
//! `EnumerateBelowThreshold` (rbsr/src/policy/enumerate_below_threshold.rs).
//!
//! The round's logic -- the shared cutoffs (policy/cutoffs.rs:21-38), the policy's stride
//! (fixed_fan_out.rs:74-80, sqrt_fan_out.rs), the cut rule (protocol/rank.rs:75-78), the
//! non-progressing SPLIT turned IDLIST (protocol.rs:263-272) -- exists once, in the library,
//! where it is checked round by round against a literal restatement of the reference's round
//! (MI355X repository: tests/test_rbsr.py, tests/test_sharded.py).  This file only converts the
//! segments to the wire codec's SoA form and the outputs back, in the reference's order.

use std::ops::Bound;
use std::os::raw::{c_int, c_void};

use rsos::{Aggregate, Fingerprint};

use crate::{check, ffi, GpuKey, RoundCounts};

/// The shipped policies the library decides on the device or its host tier: `FixedFanOut(b)`
/// (`b < 2` is raised to 2, `FanOut::new`; 16 = `FanOut::NEGENTROPY`, `protocol_round`'s default),
/// `SqrtFanOut`, and `EnumerateBelowThreshold { threshold, fan_out }` (Algorithm 1 as written:
/// IDLIST when the local span is at most `threshold`, `SPLITBYRANK(fan_out)` otherwise; a
/// `threshold` of 0 is raised to 1, `EnumerateBelowThreshold::new`).
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum RoundPolicy {
    FixedFanOut(usize),
    SqrtFanOut,
    EnumerateBelowThreshold { threshold: usize, fan_out: usize },
}

impl RoundPolicy {
    /// `EnumerateBelowThreshold::PAPER` (enumerate_below_threshold.rs:110-113): `t = 32`, `b = 16`.
    pub const PAPER: RoundPolicy = RoundPolicy::EnumerateBelowThreshold { threshold: 32, fan_out: 16 };
}

/// Which entry point a round takes, with its two leading arguments: `Policy(policy, fan_out)` is
/// `rh_[s]store_protocol_round`, `Threshold(threshold, fan_out)` `rh_[s]store_protocol_round_threshold`.
#[derive(Clone, Copy, Debug)]
pub(crate) enum RoundCall {
    Policy(c_int, u64),
    Threshold(u64, u64),
}

/// `call(which, active, children, enumerations, outcome)` makes the entry point `which` names
/// on the caller's store; the outputs it fills point into the store's own buffers, read
/// here before anything else can call the store (the caller holds its round lock).
pub(crate) fn run_round<K: GpuKey>(
    call: impl FnOnce(RoundCall, *const ffi::rh_segments, *mut ffi::rh_segments, *mut ffi::rh_segments,
                      *mut ffi::rh_round_outcome) -> c_int,
    policy: RoundPolicy,
    active: Vec<rbsr::RangeAggregate<K>>,
    child_ranges: &mut Vec<rbsr::RangeAggregate<K>>,
    enumeration_ranges: &mut Vec<rbsr::EnumerationRange<K>>,
) -> RoundCounts {
    let kl = K::LEN as usize;
    let n = active.len();
    let mut sk = vec![0u8; n.max(1)];
    let mut ek = vec![0u8; n.max(1)];
    let mut skeys = vec![0u8; n * kl + 1];
    let mut ekeys = vec![0u8; n * kl + 1];
    let mut aggs = vec![ffi::rh_aggregate::default(); n.max(1)];
    for (j, seg) in active.iter().enumerate() {
        // a RangeAggregate's start is Included or Unbounded, its end Excluded or Unbounded
        // (KeyRange, rbsr/src/protocol.rs:63-88)
        match seg.start_bound() {
            Bound::Included(k) | Bound::Excluded(k) => {
                sk[j] = 1;
                skeys[j * kl..(j + 1) * kl].copy_from_slice(&k.column_bytes());
            }
            Bound::Unbounded => {}
        }
        match seg.end_bound() {
            Bound::Included(k) | Bound::Excluded(k) => {
                ek[j] = 1;
                ekeys[j * kl..(j + 1) * kl].copy_from_slice(&k.column_bytes());
            }
            Bound::Unbounded => {}
        }
        let a = seg.aggregate();
        aggs[j] = ffi::rh_aggregate { fingerprint: a.fingerprint().0, size: a.size() as u64 };
    }
    let input = ffi::rh_segments {
        start_kinds: sk.as_mut_ptr(),
        start_keys: skeys.as_mut_ptr() as *mut c_void,
        end_kinds: ek.as_mut_ptr(),
        end_keys: ekeys.as_mut_ptr() as *mut c_void,
        aggregates: aggs.as_mut_ptr(),
        n,
        cap: n,
    };
    let which = match policy {
        RoundPolicy::FixedFanOut(b) => RoundCall::Policy(ffi::RH_POLICY_FIXED_FAN_OUT, b as u64),
        RoundPolicy::SqrtFanOut => RoundCall::Policy(ffi::RH_POLICY_SQRT_FAN_OUT, 0),
        RoundPolicy::EnumerateBelowThreshold { threshold, fan_out } => RoundCall::Threshold(threshold as u64, fan_out as u64),
    };
    let empty = ffi::rh_segments {
        start_kinds: std::ptr::null_mut(),
        start_keys: std::ptr::null_mut(),
        end_kinds: std::ptr::null_mut(),
        end_keys: std::ptr::null_mut(),
        aggregates: std::ptr::null_mut(),
        n: 0,
        cap: 0,
    };
    let (mut ch, mut en, mut oc) = (empty, empty, ffi::rh_round_outcome::default());
    check(call(which, &input, &mut ch, &mut en, &mut oc), "protocol_round");
    // SAFETY: the library filled ch / en with arrays of ch.n / en.n items (keys kl bytes each),
    // valid until the store's next call, which the caller's round lock excludes.
    unsafe {
        let key = |p: *mut c_void, i: usize| K::from_column_bytes(std::slice::from_raw_parts((p as *const u8).add(i * kl), kl));
        for i in 0..ch.n {
            let s = (*ch.start_kinds.add(i) != 0).then(|| key(ch.start_keys, i));
            let e = (*ch.end_kinds.add(i) != 0).then(|| key(ch.end_keys, i));
            let a = *ch.aggregates.add(i);
            child_ranges.push(rbsr::RangeAggregate::new(s, e, Aggregate::new(a.size as usize, Fingerprint(a.fingerprint))));
        }
        for i in 0..en.n {
            let s = if *en.start_kinds.add(i) != 0 { Bound::Included(key(en.start_keys, i)) } else { Bound::Unbounded };
            let e = if *en.end_kinds.add(i) != 0 { Bound::Excluded(key(en.end_keys, i)) } else { Bound::Unbounded };
            enumeration_ranges.push((s, e));
        }
    }
    RoundCounts {
        skipped: oc.skipped as usize,
        enumerated: oc.enumerated as usize,
        split: oc.split as usize,
        children: oc.children as usize,
        dropped_malformed: oc.dropped_malformed as usize,
    }
}

/// The keys of a round's `enumeration_ranges`, one `Vec` per range, in one store call
/// (`rh_store_enumerate_segments` / `rh_sstore_enumerate_segments`) where `Rsos::enumerate`
/// (rsos/src/rsos_trait.rs:73-83) is asked range by range.  `call(ranges, max_rows, out)` is one of
/// the two entry points on the caller's store; the answer points into the store's own buffer, read
/// here before anything else can call the store (the caller holds its round lock).  An enumeration
/// range's start is Included or Unbounded, its end Excluded or Unbounded (rbsr/src/protocol.rs).
pub(crate) fn run_enumerate<K: GpuKey>(
    call: impl FnOnce(*const ffi::rh_segments, u64, *mut ffi::rh_enumerated) -> c_int,
    ranges: &[rbsr::EnumerationRange<K>],
) -> Vec<Vec<K>> {
    let kl = K::LEN as usize;
    let n = ranges.len();
    let mut sk = vec![0u8; n.max(1)];
    let mut ek = vec![0u8; n.max(1)];
    let mut skeys = vec![0u8; n * kl + 1];
    let mut ekeys = vec![0u8; n * kl + 1];
    for (j, (start, end)) in ranges.iter().enumerate() {
        if let Bound::Included(k) | Bound::Excluded(k) = start {
            sk[j] = 1;
            skeys[j * kl..(j + 1) * kl].copy_from_slice(&k.column_bytes());
        }
        if let Bound::Included(k) | Bound::Excluded(k) = end {
            ek[j] = 1;
            ekeys[j * kl..(j + 1) * kl].copy_from_slice(&k.column_bytes());
        }
    }
    let input = ffi::rh_segments {
        start_kinds: sk.as_mut_ptr(),
        start_keys: skeys.as_mut_ptr() as *mut c_void,
        end_kinds: ek.as_mut_ptr(),
        end_keys: ekeys.as_mut_ptr() as *mut c_void,
        aggregates: std::ptr::null_mut(),
        n,
        cap: n,
    };
    let mut out = ffi::rh_enumerated {
        first_ranks: std::ptr::null(),
        offsets: std::ptr::null(),
        keys: std::ptr::null(),
        n: 0,
        rows: 0,
    };
    check(call(&input, 0, &mut out), "enumerate_segments");
    // SAFETY: the library filled out.offsets with n + 1 entries and out.keys with out.rows rows of
    // kl bytes, valid until the store's next enumerate call, which the caller's round lock excludes.
    unsafe {
        let offs = std::slice::from_raw_parts(out.offsets, n + 1);
        let rows = std::slice::from_raw_parts(out.keys as *const u8, out.rows as usize * kl);
        (0..n)
            .map(|j| (offs[j] as usize..offs[j + 1] as usize).map(|t| K::from_column_bytes(&rows[t * kl..(t + 1) * kl])).collect())
            .collect()
    }
}
