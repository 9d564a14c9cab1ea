//! Rust binding of libhbtc, the MI355X batched verifier behind hbbft's threshold-crypto calls.
//!
//! `ffi` is generated from `include/hbtc.h` (tools/gen_rust_ffi.py; tests/test_abi.py fails when
//! it drifts).  The safe layer below is what hbbft's batch queues use: a `Context` per GPU (or a
//! `Node` over several), key sets loaded once per era, and CSR-shaped batches of compressed
//! points exactly as they arrive on the wire (G1 48 bytes, G2 96 bytes).
//!
//! Call-site mapping:
//!   Coin::handle_share -> PublicKeyShare::verify          verify_sig_shares   (src/coin.rs:151)
//!   Coin::try_output   -> combine_signatures + parity     combine_sigs        (src/coin.rs:185-191)
//!   ThresholdDecryption -> verify_decryption_share        verify_dec_shares   (src/threshold_decryption.rs:159)
//!   ThresholdDecryption -> PublicKeySet::decrypt          combine_dec         (src/threshold_decryption.rs:181-185)
//!   ThresholdDecryption::try_output, to the plaintext     threshold_decrypt   (src/threshold_decryption.rs:164-188)
//!   SyncKeyGen::handle_part / handle_ack                  skg_check_parts / skg_check_acks / decrypt
//!   HoneyBadger::propose, SyncKeyGen::new / Ack values     encrypt / fr_poly_eval (src/sync_key_gen.rs:320-322,372-379)
//!   SyncKeyGen::generate + NetworkInfo::new               skg_generate        (src/sync_key_gen.rs:428-447)
//!   SyncKeyGen::new's Part / the Acks, one call each      skg_part / skg_acks (src/sync_key_gen.rs:293-330,371-380)
#![allow(clippy::too_many_arguments)]
pub mod ffi;
#[cfg(feature = "experimental-queues")]
pub mod queues;

use std::ffi::CStr;
use std::os::raw::c_int;
use std::ptr;

pub const ACCEPT: i32 = 0;
pub const REJECT: i32 = 1;
pub const DECODE_ERR: i32 = 2;
pub const UNKNOWN_SENDER: i32 = 3;
pub const INSTANCE_ERR: i32 = 4;
pub const NOT_ENOUGH_SHARES: i32 = 5;
pub const DUPLICATE_ENTRY: i32 = 6;

pub const MODE_PER_SHARE: c_int = 0;
pub const MODE_RLC: c_int = 1;

#[derive(Debug, Clone)]
pub struct Error {
    pub code: i32,
    pub message: String,
}

pub type Result<T> = std::result::Result<T, Error>;

/// A CSR batch: instance k owns items offsets[k] .. offsets[k + 1].
pub struct Batch<'a> {
    pub offsets: &'a [u32],
    pub idx: &'a [u32],
    pub items: &'a [u8],
}

impl<'a> Batch<'a> {
    fn check(&self, item_size: usize) {
        assert!(!self.offsets.is_empty() && self.offsets[0] == 0, "offsets[0] must be 0");
        assert!(self.offsets.windows(2).all(|w| w[0] <= w[1]), "offsets must be non-decreasing");
        let n = *self.offsets.last().unwrap() as usize;
        assert_eq!(self.idx.len(), n, "one node index per item");
        assert_eq!(self.items.len(), n * item_size, "item bytes");
    }
    fn n_inst(&self) -> u32 {
        (self.offsets.len() - 1) as u32
    }
    fn n_items(&self) -> usize {
        *self.offsets.last().unwrap() as usize
    }
}

/// One context on one GPU.  Calls are serialised inside the library (one mutex per context).
pub struct Context {
    raw: *mut ffi::hbtc_ctx,
}

unsafe impl Send for Context {}
unsafe impl Sync for Context {}

impl Context {
    pub fn new(device: i32) -> Result<Context> {
        let mut raw = ptr::null_mut();
        let rc = unsafe { ffi::hbtc_ctx_create(device, &mut raw) };
        if rc != 0 {
            return Err(Error { code: rc, message: format!("hbtc_ctx_create({})", device) });
        }
        Ok(Context { raw })
    }

    fn err(&self, rc: c_int) -> Error {
        let msg = unsafe { CStr::from_ptr(ffi::hbtc_last_error(self.raw)) };
        Error { code: rc, message: msg.to_string_lossy().into_owned() }
    }

    fn ok(&self, rc: c_int) -> Result<()> {
        if rc == 0 { Ok(()) } else { Err(self.err(rc)) }
    }

    /// NetworkInfo's public_key_share table (src/messaging.rs:253-256): (key set id, undecodable).
    pub fn keyset_load(&self, pk_shares_c48: &[u8]) -> Result<(u32, u32)> {
        assert_eq!(pk_shares_c48.len() % 48, 0);
        let (mut id, mut bad) = (0u32, 0u32);
        let n = (pk_shares_c48.len() / 48) as u32;
        self.ok(unsafe { ffi::hbtc_keyset_load(self.raw, pk_shares_c48.as_ptr(), n, &mut id, &mut bad) })?;
        Ok((id, bad))
    }

    pub fn keyset_free(&self, id: u32) -> Result<()> {
        self.ok(unsafe { ffi::hbtc_keyset_free(self.raw, id) })
    }

    pub fn set_verify_mode(&self, mode: c_int) -> Result<()> {
        self.ok(unsafe { ffi::hbtc_set_verify_mode(self.raw, mode) })
    }

    /// RLC scalar size: 128 (default) or 64 bits (soundness 2^-128 / 2^-64 per group check).
    pub fn set_rlc_bits(&self, bits: u32) -> Result<()> {
        self.ok(unsafe { ffi::hbtc_set_rlc_bits(self.raw, bits) })
    }

    /// Calls with fewer than `n_items` items get exact checks only, no RLC batch (default 256;
    /// 0 = always batch).  The decisions are the same either way.
    pub fn set_exact_below(&self, n_items: u32) -> Result<()> {
        self.ok(unsafe { ffi::hbtc_set_exact_below(self.raw, n_items) })
    }

    /// PublicKeyShare::verify for every SignatureShare of every coin instance (H = hash_g2(nonce)).
    pub fn verify_sig_shares(&self, keyset: u32, h_c96: &[u8], b: &Batch) -> Result<Vec<i32>> {
        b.check(96);
        assert_eq!(h_c96.len(), 96 * b.n_inst() as usize);
        let mut st = vec![0i32; b.n_items()];
        self.ok(unsafe {
            ffi::hbtc_verify_sig_shares(self.raw, keyset, b.n_inst(), h_c96.as_ptr(), b.offsets.as_ptr(),
                                        b.idx.as_ptr(), b.items.as_ptr(), st.as_mut_ptr())
        })?;
        Ok(st)
    }

    /// verify_decryption_share for every DecryptionShare (H = hash_g1_g2(u, v), w per ciphertext).
    pub fn verify_dec_shares(&self, keyset: u32, h_c96: &[u8], w_c96: &[u8], b: &Batch) -> Result<Vec<i32>> {
        b.check(48);
        assert_eq!(h_c96.len(), 96 * b.n_inst() as usize);
        assert_eq!(w_c96.len(), 96 * b.n_inst() as usize);
        let mut st = vec![0i32; b.n_items()];
        self.ok(unsafe {
            ffi::hbtc_verify_dec_shares(self.raw, keyset, b.n_inst(), h_c96.as_ptr(), w_c96.as_ptr(),
                                        b.offsets.as_ptr(), b.idx.as_ptr(), b.items.as_ptr(), st.as_mut_ptr())
        })?;
        Ok(st)
    }

    /// PublicKey::verify for n (pk, H, sigma) triples: e(pk, H) == e(G1, sigma) (src/coin.rs:192-197).
    pub fn verify_sigs(&self, pk_c48: &[u8], h_c96: &[u8], sig_c96: &[u8]) -> Result<Vec<i32>> {
        assert_eq!(pk_c48.len() % 48, 0);
        let n = pk_c48.len() / 48;
        assert_eq!(h_c96.len(), 96 * n, "one H per signature");
        assert_eq!(sig_c96.len(), 96 * n, "one signature per key");
        let mut st = vec![0i32; n];
        self.ok(unsafe {
            ffi::hbtc_verify_sigs(self.raw, n as u32, pk_c48.as_ptr(), h_c96.as_ptr(), sig_c96.as_ptr(),
                                  st.as_mut_ptr())
        })?;
        Ok(st)
    }

    /// Ciphertext::verify for n (u, H, w) triples: e(G1, w) == e(u, H) (src/threshold_decryption.rs:98).
    pub fn verify_ciphertexts(&self, u_c48: &[u8], h_c96: &[u8], w_c96: &[u8]) -> Result<Vec<i32>> {
        assert_eq!(u_c48.len() % 48, 0);
        let n = u_c48.len() / 48;
        assert_eq!(h_c96.len(), 96 * n, "one H per ciphertext");
        assert_eq!(w_c96.len(), 96 * n, "one w per ciphertext");
        let mut st = vec![0i32; n];
        self.ok(unsafe {
            ffi::hbtc_verify_ciphertexts(self.raw, n as u32, u_c48.as_ptr(), h_c96.as_ptr(), w_c96.as_ptr(),
                                         st.as_mut_ptr())
        })?;
        Ok(st)
    }

    /// BivarCommitment::row(x) == row.commitment() for every Part (x = our_idx + 1): commits holds
    /// per Part the (t+1)(t+2)/2 compressed points, rows per Part t+1 Fr (32-byte LE each).
    pub fn skg_check_parts(&self, t: u32, our_idx: u32, commits_c48: &[u8], rows_le32: &[u8]) -> Result<Vec<i32>> {
        let m = ((t + 1) * (t + 2) / 2) as usize;
        assert_eq!(commits_c48.len() % (48 * m), 0);
        let n_parts = commits_c48.len() / (48 * m);
        assert_eq!(rows_le32.len(), 32 * (t as usize + 1) * n_parts, "t + 1 row coefficients per Part");
        let mut st = vec![0i32; n_parts];
        self.ok(unsafe {
            ffi::hbtc_skg_check_parts(self.raw, n_parts as u32, t, our_idx, commits_c48.as_ptr(), rows_le32.as_ptr(),
                                      st.as_mut_ptr())
        })?;
        Ok(st)
    }

    /// BivarCommitment::evaluate(x, y) == val G1 for every Ack value (x = our_idx + 1, y = sender
    /// + 1), against Part ack_part[i]'s commitment; row_ok[p] != 0: Part p's verified row (rows)
    /// gives the scalar fast path.
    pub fn skg_check_acks(&self, t: u32, our_idx: u32, commits_c48: &[u8], rows_le32: &[u8], row_ok: &[u8],
                          ack_part: &[u32], ack_sender: &[u32], vals_le32: &[u8]) -> Result<Vec<i32>> {
        let m = ((t + 1) * (t + 2) / 2) as usize;
        assert_eq!(commits_c48.len() % (48 * m), 0);
        let n_parts = commits_c48.len() / (48 * m);
        assert_eq!(rows_le32.len(), 32 * (t as usize + 1) * n_parts);
        assert_eq!(row_ok.len(), n_parts);
        let n = ack_part.len();
        assert!(ack_part.iter().all(|&p| (p as usize) < n_parts), "ack_part out of range");
        assert_eq!(ack_sender.len(), n);
        assert_eq!(vals_le32.len(), 32 * n);
        let mut st = vec![0i32; n];
        self.ok(unsafe {
            ffi::hbtc_skg_check_acks(self.raw, n_parts as u32, t, our_idx, commits_c48.as_ptr(), rows_le32.as_ptr(),
                                     row_ok.as_ptr(), n as u32, ack_part.as_ptr(), ack_sender.as_ptr(),
                                     vals_le32.as_ptr(), st.as_mut_ptr())
        })?;
        Ok(st)
    }

    /// combine_signatures over the first t shares of every instance: (signatures, parities, status).
    pub fn combine_sigs(&self, b: &Batch, t: u32) -> Result<(Vec<u8>, Vec<u8>, Vec<i32>)> {
        b.check(96);
        let n = b.n_inst() as usize;
        let (mut out, mut par, mut st) = (vec![0u8; 96 * n], vec![0u8; n], vec![0i32; n]);
        self.ok(unsafe {
            ffi::hbtc_combine_sigs(self.raw, b.n_inst(), b.offsets.as_ptr(), b.idx.as_ptr(), b.items.as_ptr(), t,
                                   out.as_mut_ptr(), par.as_mut_ptr(), st.as_mut_ptr())
        })?;
        Ok((out, par, st))
    }

    /// PublicKeySet::decrypt's interpolation: g per ciphertext (plaintext = v ^ hash_bytes(g)).
    pub fn combine_dec(&self, b: &Batch, t: u32) -> Result<(Vec<u8>, Vec<i32>)> {
        b.check(48);
        let n = b.n_inst() as usize;
        let (mut out, mut st) = (vec![0u8; 48 * n], vec![0i32; n]);
        self.ok(unsafe {
            ffi::hbtc_combine_dec(self.raw, b.n_inst(), b.offsets.as_ptr(), b.idx.as_ptr(), b.items.as_ptr(), t,
                                  out.as_mut_ptr(), st.as_mut_ptr())
        })?;
        Ok((out, st))
    }

    /// One ThresholdDecryption round (try_output, src/threshold_decryption.rs:164-188): the shares of
    /// `b` verified against (h, w), the first t ACCEPTed shares of every ciphertext combined and the
    /// plaintext v ^ hash_bytes(g, |v|) made on the GPU.  v holds ciphertext k's v at
    /// v_offsets[k] .. v_offsets[k + 1].  Returns (share status, g, plaintexts in v's layout,
    /// ciphertext status); a ciphertext that is not ACCEPT has zeros for g and for its plaintext.
    pub fn threshold_decrypt(&self, keyset: u32, h_c96: &[u8], w_c96: &[u8], b: &Batch, t: u32, v: &[u8],
                             v_offsets: &[u32]) -> Result<(Vec<i32>, Vec<u8>, Vec<u8>, Vec<i32>)> {
        b.check(48);
        let n = b.n_inst() as usize;
        assert_eq!(h_c96.len(), 96 * n, "one compressed G2 H per ciphertext");
        assert_eq!(w_c96.len(), 96 * n, "one compressed G2 w per ciphertext");
        assert!(t >= 1, "t must be >= 1");
        assert_eq!(v_offsets.len(), n + 1, "one v per ciphertext");
        assert!(v_offsets[0] == 0 && v_offsets.windows(2).all(|w| w[0] <= w[1]), "v_offsets must start at 0 and not decrease");
        assert!(v_offsets[n] as usize <= v.len(), "v_offsets past the bytes of v");
        let (mut st, mut g) = (vec![0i32; b.idx.len()], vec![0u8; 48 * n]);
        let (mut plain, mut cst) = (vec![0u8; v.len()], vec![0i32; n]);
        self.ok(unsafe {
            ffi::hbtc_threshold_decrypt(self.raw, keyset, b.n_inst(), h_c96.as_ptr(), w_c96.as_ptr(), b.offsets.as_ptr(),
                                        b.idx.as_ptr(), b.items.as_ptr(), t, v.as_ptr(), v_offsets.as_ptr(),
                                        st.as_mut_ptr(), g.as_mut_ptr(), plain.as_mut_ptr(), cst.as_mut_ptr())
        })?;
        Ok((st, g, plain, cst))
    }

    /// SecretKey::decrypt for a batch under one key: (plaintexts in the msgs layout, status).
    pub fn decrypt(&self, sk_le32: &[u8; 32], u_c48: &[u8], w_c96: &[u8], msgs: &[u8], offsets: &[u32])
        -> Result<(Vec<u8>, Vec<i32>)> {
        assert!(!offsets.is_empty() && offsets[0] == 0, "offsets[0] must be 0");
        assert!(offsets.windows(2).all(|w| w[0] <= w[1]), "offsets must be non-decreasing");
        let n = offsets.len() - 1;
        assert!(offsets[n] as usize <= msgs.len(), "offsets past the message bytes");
        assert_eq!(u_c48.len(), 48 * n, "one compressed G1 u per ciphertext");
        assert_eq!(w_c96.len(), 96 * n, "one compressed G2 w per ciphertext");
        let (mut out, mut st) = (vec![0u8; msgs.len()], vec![0i32; n]);
        self.ok(unsafe {
            ffi::hbtc_decrypt(self.raw, n as u32, sk_le32.as_ptr(), u_c48.as_ptr(), w_c96.as_ptr(), msgs.as_ptr(),
                              offsets.as_ptr(), out.as_mut_ptr(), st.as_mut_ptr())
        })?;
        Ok((out, st))
    }

    /// PublicKey::encrypt_with_rng for a batch: (u, v in the msgs layout, w, status).  pk_c48 holds
    /// one key per item, or a single key shared by all (48 bytes).
    pub fn encrypt(&self, pk_c48: &[u8], r_le32: &[u8], msgs: &[u8], offsets: &[u32])
        -> Result<(Vec<u8>, Vec<u8>, Vec<u8>, Vec<i32>)> {
        assert!(!offsets.is_empty() && offsets[0] == 0, "offsets[0] must be 0");
        assert!(offsets.windows(2).all(|w| w[0] <= w[1]), "offsets must be non-decreasing");
        let n = offsets.len() - 1;
        assert!(offsets[n] as usize <= msgs.len(), "offsets past the message bytes");
        assert_eq!(r_le32.len(), 32 * n, "one 32-byte scalar per item");
        assert!(pk_c48.len() == 48 * n || pk_c48.len() == 48, "one key per item, or one shared key");
        let stride = if pk_c48.len() == 48 * n { 1 } else { 0 };
        let (mut u, mut v, mut w, mut st) = (vec![0u8; 48 * n], vec![0u8; msgs.len()], vec![0u8; 96 * n], vec![0i32; n]);
        self.ok(unsafe {
            ffi::hbtc_encrypt(self.raw, n as u32, pk_c48.as_ptr(), stride, r_le32.as_ptr(), msgs.as_ptr(),
                              offsets.as_ptr(), u.as_mut_ptr(), v.as_mut_ptr(), w.as_mut_ptr(), st.as_mut_ptr())
        })?;
        Ok((u, v, w, st))
    }

    /// SecretKeyShare::decrypt_share for a batch under one secret key share
    /// (ThresholdDecryption::set_ciphertext, src/threshold_decryption.rs:94-113): (shares, H, status).
    /// H[96 i ..] = hash_g1_g2(u_i, v_i) for every item; shares[48 i ..] = sk u_i where status[i] is
    /// ACCEPT and 48 zero bytes elsewhere (REJECT: decrypt_share returns None).  Written against the
    /// C ABI and, like the rest of this crate, not compiled in this repository's checks.
    pub fn decrypt_shares(&self, sk_le32: &[u8; 32], u_c48: &[u8], v: &[u8], v_offsets: &[u32], w_c96: &[u8])
        -> Result<(Vec<u8>, Vec<u8>, Vec<i32>)> {
        assert!(!v_offsets.is_empty() && v_offsets[0] == 0, "v_offsets[0] must be 0");
        assert!(v_offsets.windows(2).all(|w| w[0] <= w[1]), "v_offsets must be non-decreasing");
        let n = v_offsets.len() - 1;
        assert!(v_offsets[n] as usize <= v.len(), "v_offsets past the bytes of v");
        assert_eq!(u_c48.len(), 48 * n, "one compressed G1 u per ciphertext");
        assert_eq!(w_c96.len(), 96 * n, "one compressed G2 w per ciphertext");
        let (mut g, mut h, mut st) = (vec![0u8; 48 * n], vec![0u8; 96 * n], vec![0i32; n]);
        self.ok(unsafe {
            ffi::hbtc_decrypt_shares(self.raw, n as u32, sk_le32.as_ptr(), u_c48.as_ptr(), v.as_ptr(),
                                     v_offsets.as_ptr(), w_c96.as_ptr(), g.as_mut_ptr(), h.as_mut_ptr(),
                                     st.as_mut_ptr())
        })?;
        Ok((g, h, st))
    }

    /// SecretKeyShare::sign for a batch of messages under one secret key (share) (Coin::get_coin,
    /// src/coin.rs:142): (signatures, H) with H[96 i ..] = hash_g2(msg_i) and sig_i = sk H_i.
    pub fn sign_shares(&self, sk_le32: &[u8; 32], msgs: &[u8], offsets: &[u32]) -> Result<(Vec<u8>, Vec<u8>)> {
        assert!(!offsets.is_empty() && offsets[0] == 0, "offsets[0] must be 0");
        assert!(offsets.windows(2).all(|w| w[0] <= w[1]), "offsets must be non-decreasing");
        let n = offsets.len() - 1;
        assert!(offsets[n] as usize <= msgs.len(), "offsets past the message bytes");
        let (mut sig, mut h) = (vec![0u8; 96 * n], vec![0u8; 96 * n]);
        self.ok(unsafe {
            ffi::hbtc_sign_shares(self.raw, n as u32, sk_le32.as_ptr(), msgs.as_ptr(), offsets.as_ptr(),
                                  sig.as_mut_ptr(), h.as_mut_ptr())
        })?;
        Ok((sig, h))
    }

    /// PublicKey::verify of DynamicHoneyBadger's signed votes and key-generation messages
    /// (src/dynamic_honey_badger/votes.rs:150-155, dynamic_honey_badger.rs:425-440), grouped by signer:
    /// `signer[i]` indexes the key set (the validators' public keys, a candidate's appended), message i
    /// is msgs[offsets[i] .. offsets[i + 1]), `sig_c96` holds one 96-byte signature per message.
    /// Returns one HBTC_* status per message.
    pub fn verify_signed_msgs(&self, keyset_id: u32, signer: &[u32], msgs: &[u8], offsets: &[u32],
                              sig_c96: &[u8]) -> Result<Vec<i32>> {
        assert!(!offsets.is_empty() && offsets[0] == 0, "offsets[0] must be 0");
        assert!(offsets.windows(2).all(|w| w[0] <= w[1]), "offsets must be non-decreasing");
        let n = offsets.len() - 1;
        assert!(offsets[n] as usize <= msgs.len(), "offsets past the message bytes");
        assert_eq!(signer.len(), n, "one signer per message");
        assert_eq!(sig_c96.len(), 96 * n, "one 96-byte signature per message");
        let mut status = vec![0i32; n];
        self.ok(unsafe {
            ffi::hbtc_verify_signed_msgs(self.raw, keyset_id, n as u32, signer.as_ptr(), msgs.as_ptr(),
                                         offsets.as_ptr(), sig_c96.as_ptr(), status.as_mut_ptr())
        })?;
        Ok(status)
    }

    /// out[p * n_x + j] = poly_p(x_j) over Fr (32-byte LE each): n_poly rows of n_coeff coefficients.
    pub fn fr_poly_eval(&self, n_coeff: u32, coeffs_le32: &[u8], x_le32: &[u8]) -> Result<Vec<u8>> {
        assert_eq!(x_le32.len() % 32, 0);
        let n_x = x_le32.len() / 32;
        let row = 32 * n_coeff as usize;
        assert!(row > 0 && coeffs_le32.len() % row == 0, "n_coeff coefficients per polynomial");
        let n_poly = coeffs_le32.len() / row;
        let mut out = vec![0u8; 32 * n_poly * n_x];
        self.ok(unsafe {
            ffi::hbtc_fr_poly_eval(self.raw, n_poly as u32, n_coeff, coeffs_le32.as_ptr(), n_x as u32,
                                   x_le32.as_ptr(), out.as_mut_ptr())
        })?;
        Ok(out)
    }

    /// SyncKeyGen::generate + NetworkInfo::new in one call (written against the C ABI and, like the
    /// rest of this crate, not compiled in this repository's checks).  `row0_c48`: coefficient
    /// (0, j) of every complete Part's commitment, Part-major, t + 1 points each.  `values`: the
    /// stored values as (CSR offsets over the Parts, x = sender index + 1, 32-byte LE values), or
    /// None for an observer.  With `load_keyset` the n_nodes shares become a loaded key set whose
    /// master key is the commitment's constant term.  On a status other than ACCEPT the outputs
    /// are zero-filled and no key set exists.
    pub fn skg_generate(&self, t: u32, row0_c48: &[u8], values: Option<(&[u32], &[u32], &[u8])>,
                        n_nodes: u32, load_keyset: bool) -> Result<GeneratedKeys> {
        let t1 = t as usize + 1;
        assert!(!row0_c48.is_empty() && row0_c48.len() % (48 * t1) == 0, "t + 1 points per Part");
        let n_parts = row0_c48.len() / (48 * t1);
        if let Some((off, x, v)) = values {
            assert_eq!(off.len(), n_parts + 1, "one offset per Part and the end");
            assert!(off[0] == 0 && off.windows(2).all(|w| w[0] <= w[1]), "offsets start at 0 and do not decrease");
            let n = off[n_parts] as usize;
            assert!(x.len() == n && v.len() == 32 * n, "one x and one 32-byte value per stored value");
        }
        let mut commit = vec![0u8; 48 * t1];
        let mut pk_shares = vec![0u8; 48 * n_nodes as usize];
        let mut sk = [0u8; 32];
        let (mut id, mut status) = (0u32, -1i32);
        let (off_p, x_p, v_p, sk_p) = match values {
            Some((off, x, v)) => (off.as_ptr(), x.as_ptr(), v.as_ptr(), sk.as_mut_ptr()),
            None => (ptr::null(), ptr::null(), ptr::null(), ptr::null_mut()),
        };
        self.ok(unsafe {
            ffi::hbtc_skg_generate(self.raw, n_parts as u32, t, row0_c48.as_ptr(), off_p, x_p, v_p, n_nodes,
                                   commit.as_mut_ptr(),
                                   if n_nodes > 0 { pk_shares.as_mut_ptr() } else { ptr::null_mut() }, sk_p,
                                   if load_keyset { &mut id } else { ptr::null_mut() }, &mut status)
        })?;
        Ok(GeneratedKeys {
            commit,
            pk_shares,
            sk: values.map(|_| sk),
            keyset_id: if load_keyset && status == ACCEPT { Some(id) } else { None },
            status,
        })
    }

    /// SyncKeyGen::new's Part in one call (src/sync_key_gen.rs:293-330; written against the C ABI
    /// and, like the rest of this crate, not compiled in this repository's checks).  The recipients
    /// are the `n_nodes` keys of the loaded key set `keyset_id`.  `bcoef_le32`: the
    /// (t + 1)(t + 2) / 2 packed coefficients; `r_le32`: one encryption scalar per node.  Returns
    /// (commitment, u, v with 8 + 40 (t + 1) bytes per node, w, status).
    pub fn skg_part(&self, keyset_id: u32, n_nodes: usize, t: u32, bcoef_le32: &[u8], r_le32: &[u8])
        -> Result<(Vec<u8>, Vec<u8>, Vec<u8>, Vec<u8>, Vec<i32>)> {
        let t1 = t as usize + 1;
        let m = t1 * (t1 + 1) / 2;
        assert_eq!(bcoef_le32.len(), 32 * m, "(t + 1)(t + 2) / 2 coefficients");
        assert_eq!(r_le32.len(), 32 * n_nodes, "one 32-byte scalar per node");
        let mut commit = vec![0u8; 48 * m];
        let (mut u, mut v, mut w, mut st) =
            (vec![0u8; 48 * n_nodes], vec![0u8; (8 + 40 * t1) * n_nodes], vec![0u8; 96 * n_nodes], vec![0i32; n_nodes]);
        self.ok(unsafe {
            ffi::hbtc_skg_part(self.raw, keyset_id, t, bcoef_le32.as_ptr(), r_le32.as_ptr(), commit.as_mut_ptr(),
                               u.as_mut_ptr(), v.as_mut_ptr(), w.as_mut_ptr(), st.as_mut_ptr())
        })?;
        Ok((commit, u, v, w, st))
    }

    /// The Acks of verified Parts in one call per chunk of whole rows (src/sync_key_gen.rs:371-380;
    /// not compiled in this repository's checks either).  `rows_le32`: rows of `n_coeff`
    /// coefficients; `r_le32`: one scalar per (row, node).  Item a * n_nodes + i is row a's value at
    /// i + 1 encrypted to node i.  Returns (u, v with 40 bytes per item, w, status).
    pub fn skg_acks(&self, keyset_id: u32, n_nodes: usize, n_coeff: u32, rows_le32: &[u8], r_le32: &[u8])
        -> Result<(Vec<u8>, Vec<u8>, Vec<u8>, Vec<i32>)> {
        assert!(n_nodes > 0 && n_nodes <= SKG_ACKS_MAX_ITEMS, "between 1 and 2^20 nodes");
        assert_eq!(r_le32.len() % (32 * n_nodes), 0, "one 32-byte scalar per row and node");
        let n_rows = r_le32.len() / (32 * n_nodes);
        let row = 32 * n_coeff as usize;
        assert_eq!(rows_le32.len(), row * n_rows, "n_coeff coefficients per row");
        let n = n_rows * n_nodes;
        let (mut u, mut v, mut w, mut st) = (vec![0u8; 48 * n], vec![0u8; 40 * n], vec![0u8; 96 * n], vec![0i32; n]);
        let per = SKG_ACKS_MAX_ITEMS / n_nodes;
        let mut a0 = 0;
        while a0 < n_rows {
            let a1 = n_rows.min(a0 + per);
            let i0 = a0 * n_nodes;
            self.ok(unsafe {
                ffi::hbtc_skg_acks(self.raw, keyset_id, (a1 - a0) as u32, n_coeff,
                                   if row > 0 { rows_le32[row * a0..].as_ptr() } else { ptr::null() },
                                   r_le32[32 * i0..].as_ptr(), u[48 * i0..].as_mut_ptr(), v[40 * i0..].as_mut_ptr(),
                                   w[96 * i0..].as_mut_ptr(), st[i0..].as_mut_ptr())
            })?;
            a0 = a1;
        }
        Ok((u, v, w, st))
    }
}

/// Items of one `hbtc_skg_acks` call; `Context::skg_acks` splits a larger batch by whole rows.
pub const SKG_ACKS_MAX_ITEMS: usize = 1 << 20;

/// What `Context::skg_generate` returns: the PublicKeySet's commitment (t + 1 compressed G1), every
/// node's public key share, our secret key share (None for an observer), the loaded key set.
pub struct GeneratedKeys {
    pub commit: Vec<u8>,
    pub pk_shares: Vec<u8>,
    pub sk: Option<[u8; 32]>,
    pub keyset_id: Option<u32>,
    pub status: i32,
}

impl Drop for Context {
    fn drop(&mut self) {
        unsafe { ffi::hbtc_ctx_destroy(self.raw) }
    }
}

/// One hbbft node over several GPUs (strong scaling of one epoch).
pub struct Node {
    raw: *mut ffi::hbtc_node,
}

unsafe impl Send for Node {}
unsafe impl Sync for Node {}

impl Node {
    pub fn new(devices: &[i32]) -> Result<Node> {
        let mut raw = ptr::null_mut();
        let rc = unsafe { ffi::hbtc_node_create(devices.len() as c_int, devices.as_ptr(), &mut raw) };
        if rc != 0 {
            return Err(Error { code: rc, message: "hbtc_node_create".into() });
        }
        Ok(Node { raw })
    }

    fn ok(&self, rc: c_int) -> Result<()> {
        if rc == 0 {
            return Ok(());
        }
        let msg = unsafe { CStr::from_ptr(ffi::hbtc_node_last_error(self.raw)) };
        Err(Error { code: rc, message: msg.to_string_lossy().into_owned() })
    }

    pub fn keyset_load(&self, pk_shares_c48: &[u8]) -> Result<(u32, u32)> {
        assert_eq!(pk_shares_c48.len() % 48, 0);
        let (mut id, mut bad) = (0u32, 0u32);
        self.ok(unsafe {
            ffi::hbtc_node_keyset_load(self.raw, pk_shares_c48.as_ptr(), (pk_shares_c48.len() / 48) as u32, &mut id,
                                       &mut bad)
        })?;
        Ok((id, bad))
    }

    pub fn verify_dec_shares(&self, keyset: u32, h_c96: &[u8], w_c96: &[u8], b: &Batch) -> Result<Vec<i32>> {
        b.check(48);
        assert_eq!(h_c96.len(), 96 * b.n_inst() as usize);
        assert_eq!(w_c96.len(), 96 * b.n_inst() as usize);
        let mut st = vec![0i32; b.n_items()];
        self.ok(unsafe {
            ffi::hbtc_node_verify_dec_shares(self.raw, keyset, b.n_inst(), h_c96.as_ptr(), w_c96.as_ptr(),
                                             b.offsets.as_ptr(), b.idx.as_ptr(), b.items.as_ptr(), st.as_mut_ptr())
        })?;
        Ok(st)
    }

    pub fn verify_sig_shares(&self, keyset: u32, h_c96: &[u8], b: &Batch) -> Result<Vec<i32>> {
        b.check(96);
        assert_eq!(h_c96.len(), 96 * b.n_inst() as usize);
        let mut st = vec![0i32; b.n_items()];
        self.ok(unsafe {
            ffi::hbtc_node_verify_sig_shares(self.raw, keyset, b.n_inst(), h_c96.as_ptr(), b.offsets.as_ptr(),
                                             b.idx.as_ptr(), b.items.as_ptr(), st.as_mut_ptr())
        })?;
        Ok(st)
    }
}

impl Drop for Node {
    fn drop(&mut self) {
        unsafe { ffi::hbtc_node_destroy(self.raw) }
    }
}

/// threshold_crypto's hash_g2(msg) (host).
pub fn hash_g2(msg: &[u8]) -> [u8; 96] {
    let mut out = [0u8; 96];
    unsafe { ffi::hbtc_hash_g2(msg.as_ptr(), msg.len(), out.as_mut_ptr()) };
    out
}
