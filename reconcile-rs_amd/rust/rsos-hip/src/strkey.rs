//! Short string keys for the column store: `RH_KEY_STR` (include/rsos_hip.h).
//!
//! A `String` / `Vec<u8>` key has no fixed width, so a map keyed by one used to be a
//! [`crate::HipEncodedMap`].  A string of at most `W - 1` bytes fits a `W`-byte key row -- its
//! bytes, zero padding up to offset `W - 2`, its length in byte `W - 1` -- whose `memcmp` order is
//! the strings' `Ord`: bytes decide first; a proper prefix comes first, because the padding is the
//! minimum byte; strings that tie over all `W - 1` bytes differ only in trailing zero bytes and
//! are ordered by the length byte.  The device sorts, searches and merges such rows as
//! `[u8; W]` keys; only the lift hashes the string -- u64 length, then the bytes
//! (rsos/src/encoding/serializer.rs:105-113) -- so the fingerprints are those of the reference's
//! map over `String` / `Vec<u8>` keys.  Longer strings stay with the encoded map.
//!
//! Values under such keys: `String` / `Vec<u8>` (VARBYTES) and the `FixedValue` types `()`, `u32` /
//! `i32`, `u64` / `i64`, plain or inside `Entry<Timestamp, V>` / `State<V>`; batches of a
//! string-keyed map of any size take the library's large-batch route (its one-launch small-batch
//! kernels hash the row, not the string).
use serde::{Deserialize, Deserializer, Serialize, Serializer};

use crate::{ffi, GpuKey};

/// A byte string of at most `W - 1` bytes, `W` = 16, 32 or 64.  `Ord` is the bytes' (that of
/// `Vec<u8>` / `String`), and agrees with the `memcmp` order of [`ShortString::pack`]'s rows.  It
/// serialises exactly as a `Vec<u8>` of the same bytes -- for rsos's canonical encoder and for
/// bincode the bytes a `String` of that content gives too.
#[derive(Clone, Debug, Default, PartialEq, Eq, Hash, PartialOrd, Ord)]
pub struct ShortString<const W: usize>(Vec<u8>);

impl<const W: usize> ShortString<W> {
    /// The longest string a row holds.
    pub const MAX: usize = W - 1;

    /// `None` for more than `W - 1` bytes.
    pub fn new(bytes: impl Into<Vec<u8>>) -> Option<Self> {
        let b = bytes.into();
        (b.len() <= Self::MAX).then_some(ShortString(b))
    }
    pub fn as_bytes(&self) -> &[u8] {
        &self.0
    }
    /// The string, when its bytes are UTF-8.
    pub fn as_str(&self) -> Option<&str> {
        std::str::from_utf8(&self.0).ok()
    }
    pub fn into_vec(self) -> Vec<u8> {
        self.0
    }
    /// The key row: the bytes, zero padding, the length in the last byte.
    pub fn pack(&self) -> [u8; W] {
        let mut row = [0u8; W];
        row[..self.0.len()].copy_from_slice(&self.0);
        row[W - 1] = self.0.len() as u8;
        row
    }
    /// `pack`'s inverse; `None` for a length byte above `W - 1` or nonzero padding.
    pub fn unpack(row: &[u8]) -> Option<Self> {
        if row.len() != W {
            return None;
        }
        let len = row[W - 1] as usize;
        if len > Self::MAX || row[len..W - 1].iter().any(|&b| b != 0) {
            return None;
        }
        Some(ShortString(row[..len].to_vec()))
    }
}

impl<const W: usize> TryFrom<&str> for ShortString<W> {
    type Error = usize;
    /// `Err(len)` for a string of more than `W - 1` bytes.
    fn try_from(s: &str) -> Result<Self, usize> {
        Self::new(s.as_bytes()).ok_or(s.len())
    }
}

impl<const W: usize> TryFrom<String> for ShortString<W> {
    type Error = usize;
    fn try_from(s: String) -> Result<Self, usize> {
        let len = s.len();
        Self::new(s.into_bytes()).ok_or(len)
    }
}

impl<const W: usize> Serialize for ShortString<W> {
    fn serialize<S: Serializer>(&self, s: S) -> Result<S::Ok, S::Error> {
        self.0.serialize(s) // Vec<u8>'s own impl: the length, then the bytes
    }
}

impl<'de, const W: usize> Deserialize<'de> for ShortString<W> {
    fn deserialize<D: Deserializer<'de>>(d: D) -> Result<Self, D::Error> {
        let v = Vec::<u8>::deserialize(d)?;
        let len = v.len();
        ShortString::new(v).ok_or_else(|| serde::de::Error::invalid_length(len, &"at most W - 1 bytes"))
    }
}

macro_rules! short_string_key {
    ($($w:literal)*) => {$(
        impl GpuKey for ShortString<$w> {
            const KIND: i32 = ffi::RH_KEY_STR;
            const LEN: u32 = $w;
            fn column_bytes(&self) -> Vec<u8> { self.pack().to_vec() }
            fn from_column_bytes(b: &[u8]) -> Self { Self::unpack(b).expect("a RH_KEY_STR key row") }
        }
    )*};
}
short_string_key!(16 32 64);

#[cfg(test)]
mod tests {
    use super::*;

    #[test]
    fn fixed_width_values_under_string_keys() {
        use crate::{schema, RecordRow};
        use crate::GpuRecord;
        use lww_register::{Entry, State, Timestamp};
        let s = schema::<ShortString<16>, u32>();
        assert_eq!((s.key_kind, s.key_len, s.value_kind, s.value_len, s.record_kind),
                   (ffi::RH_KEY_STR, 16, ffi::RH_VAL_U32, 4, ffi::RH_REC_PLAIN));
        let s = schema::<ShortString<32>, Entry<Timestamp, i64>>();
        assert_eq!((s.key_len, s.value_kind, s.value_len, s.record_kind), (32, ffi::RH_VAL_U64, 8, ffi::RH_REC_DATED));
        let s = schema::<ShortString<64>, State<()>>();
        assert_eq!((s.key_len, s.value_kind, s.value_len, s.record_kind), (64, ffi::RH_VAL_UNIT, 0, ffi::RH_REC_PROJECTION));
        let s = schema::<ShortString<64>, ()>();
        assert_eq!((s.value_kind, s.value_len, s.record_kind), (ffi::RH_VAL_UNIT, 0, ffi::RH_REC_PLAIN));
        let mut row = RecordRow::default();
        (-2i32).write(&mut row);
        assert_eq!(row.value, vec![0xfe, 0xff, 0xff, 0xff]);
        let mut row = RecordRow::default();
        ().write(&mut row);
        assert!(row.value.is_empty());
    }

    #[test]
    fn row_order_is_string_order() {
        let strs: Vec<&[u8]> = vec![b"", b"\0", b"\0\0", b"a", b"a\0", b"a\0\0", b"a\x01", b"ab", b"b", &[0xff; 31], &[0xff; 30]];
        let mut keys: Vec<ShortString<32>> = strs.iter().map(|s| ShortString::new(*s).unwrap()).collect();
        let mut rows: Vec<[u8; 32]> = keys.iter().map(|k| k.pack()).collect();
        keys.sort();
        rows.sort();
        assert_eq!(rows, keys.iter().map(|k| k.pack()).collect::<Vec<_>>());
        assert!(keys.iter().all(|k| ShortString::<32>::unpack(&k.pack()).as_ref() == Some(k)));
        assert!(ShortString::<32>::new(vec![0u8; 32]).is_none());
        assert!(ShortString::<16>::try_from("exactly 16 bytes").is_err());
    }

    #[test]
    fn row_order_is_string_order_at_64() {
        let long = [b'k'; 63];
        let mut other = long;
        other[62] = b'l';
        let zeros = [0u8; 63];
        let strs: Vec<&[u8]> = vec![
            b"", b"\0", b"\0\0", &zeros[..62], &zeros, b"a", b"a\0", b"a\x01", b"ab", &long[..62], &long, &other,
            &[0xff; 62], &[0xff; 63], b"namespace/ReplicaSet/frontend-web-7c9d8b6f54-x7k2p",
        ];
        let mut keys: Vec<ShortString<64>> = strs.iter().map(|s| ShortString::new(*s).unwrap()).collect();
        let mut rows: Vec<[u8; 64]> = keys.iter().map(|k| k.pack()).collect();
        keys.sort();
        rows.sort();
        assert_eq!(rows, keys.iter().map(|k| k.pack()).collect::<Vec<_>>());
        assert!(keys.iter().all(|k| ShortString::<64>::unpack(&k.pack()).as_ref() == Some(k)));
        assert_eq!(ShortString::<64>::MAX, 63);
        assert!(ShortString::<64>::new(vec![0u8; 64]).is_none());
        let mut bad = ShortString::<64>::new(&b"abc"[..]).unwrap().pack();
        bad[63] = 64;
        assert!(ShortString::<64>::unpack(&bad).is_none());
    }
}
