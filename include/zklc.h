/* zklc.h -- C ABI of libzklc_mi355.so: MI355X (gfx950) kernels for the NEAR
 * zk-light-client signature-aggregation hot path.
 *
 * The reference (ZpokenWeb3/zk-light-client-implementation) has no FFI for this
 * path; each entry point names the reference interface it replaces
 * (paths relative to the reference root) and INTEGRATION.md shows the Rust
 * `extern "C"` / cgo binding a maintainer would add at that call site.
 *
 * Conventions
 *   - all integers little-endian; status = int32_t, 0 = ZKLC_OK, negative = error
 *   - `*_dev` entry points take DEVICE pointers plus a hipStream_t (as void*;
 *     NULL = HIP's legacy default stream, as everywhere in HIP) and only
 *     enqueue work on that stream;
 *     the plain entry points take caller-owned HOST pointers, stage through the
 *     context's device buffers and return after the result is on the host.
 *   - never aborts, never unwinds across the boundary; re-entrant per context
 *     (one context per host thread / per process-per-GPU rank).
 */
#ifndef ZKLC_H
#define ZKLC_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct zklc_ctx zklc_ctx;

#define ZKLC_OK 0
#define ZKLC_ERR_INVALID_ARG (-1)
#define ZKLC_ERR_OOM (-2)
#define ZKLC_ERR_HIP (-3)
#define ZKLC_ERR_NO_DEVICE (-4)
#define ZKLC_ERR_IO (-5)        /* a container file could not be opened / written (errno is the caller's to read) */
#define ZKLC_ERR_FORMAT (-6)    /* not a container, another version, truncated, a failed checksum or sections that contradict each other */
#define ZKLC_ERR_NOT_FOUND (-7) /* the container has no section with that tag */

/* One context per process-per-GPU rank.  Owns a stream, staging buffers and
 * the constant tables (Ed25519 base-point table, NTT twiddles, ...). */
int32_t zklc_init(zklc_ctx **out, int32_t device_id);
/* same, with the context's stream created at the device's highest stream priority when `high_priority` != 0: for the short,
 * latency-critical proofs of a dependent chain (the fold of signatures.rs:97-105) sharing the GPU with long throughput work */
int32_t zklc_init_priority(zklc_ctx **out, int32_t device_id, int32_t high_priority);
void zklc_destroy(zklc_ctx *ctx);
const char *zklc_strerror(int32_t code);
/* last HIP error string seen by this context (for ZKLC_ERR_HIP) */
const char *zklc_last_hip_error(zklc_ctx *ctx);
int32_t zklc_synchronize(zklc_ctx *ctx);
/* the context's own non-blocking hipStream_t (what the host-pointer entry points run on); pass it to the *_dev entry
 * points to keep several contexts' work concurrent on one GPU */
void *zklc_stream(zklc_ctx *ctx);
uint32_t zklc_abi_version(void);
/* Device memory for hosts that bind nothing but this ABI (a C / Rust / Go caller need not link the HIP runtime to hold the
 * buffers the *_dev entry points take): alloc returns a ZERO-FILLED buffer on the context's GPU (what
 * zklc_plonky2_witness_run_dev expects of d_wires); copy moves bytes between host and device on the context's stream and returns
 * when they have arrived (to_host != 0: device -> host). */
int32_t zklc_device_alloc(zklc_ctx *ctx, uint64_t bytes, void **d_out);
int32_t zklc_device_free(zklc_ctx *ctx, void *d_ptr);
int32_t zklc_device_copy(zklc_ctx *ctx, void *dst, const void *src, uint64_t bytes, int32_t to_host);

/* ---- (a) batched Ed25519 -------------------------------------------------
 * Replaces the per-approval native pre-check loop
 *   near_bft_finality/src/prove_block_data/signatures.rs:70-123 (`sig.verify(msg,&pk)` :79)
 * and the in-tree restatement crypto/plonky2_ed25519/src/curve/eddsa.rs:33-58.
 * pks: n*32 bytes, sigs: n*64 bytes (R || s).  Message: msg_stride == 0 ->
 * one msg_len-byte message shared by all n signatures (NEAR: every validator
 * signs the same Approval bytes, signatures.rs:24-39); otherwise signature i
 * uses msgs + i*msg_stride.  ok[i] = 1 valid / 0 invalid (ed25519-dalek
 * non-strict semantics: s >= l rejected, undecodable A rejected,
 * compress([s]B - [h]A) == R bytes). */
int32_t zklc_ed25519_verify_batch(zklc_ctx *ctx, const uint8_t *pks, const uint8_t *sigs, const uint8_t *msgs,
                                  uint32_t msg_len, uint32_t msg_stride, uint32_t n, uint8_t *ok);
int32_t zklc_ed25519_verify_batch_dev(zklc_ctx *ctx, void *stream, const uint8_t *d_pks, const uint8_t *d_sigs,
                                      const uint8_t *d_msgs, uint32_t msg_len, uint32_t msg_stride, uint32_t n,
                                      uint8_t *d_ok);

/* SHA-512 of n equal-length messages (in + i*stride, len bytes) -> out + 64*i.
 * Replaces sha2::Sha512 at crypto/plonky2_ed25519/src/curve/eddsa.rs:40-42 and
 * the witness side of crypto/plonky2_sha512/src/circuit.rs:308-435. */
int32_t zklc_sha512_batch(zklc_ctx *ctx, const uint8_t *in, uint32_t stride, uint32_t len, uint32_t n, uint8_t *out);
int32_t zklc_sha512_batch_dev(zklc_ctx *ctx, void *stream, const uint8_t *d_in, uint32_t stride, uint32_t len,
                              uint32_t n, uint8_t *d_out);

/* ---- (b) Goldilocks: NTT / LDE / Poseidon / Merkle --------------------------
 * Replace the prover internals of the un-vendored plonky2 fork
 * (wormhole-foundation/plonky2-near@2244a9d, Cargo.toml:44-47) reached from
 * `circuit_data.prove(pw)` at near_bft_finality/src/prove_crypto/ed25519.rs:60,100
 * and recursion.rs:95: `fft`/`ifft`/`coset_fft` (plonky2_field::fft),
 * `PolynomialBatch::from_coeffs` (LDE + Merkle) and `MerkleTree::new`.
 * Elements are canonical u64 < p = 2^64 - 2^32 + 1.  A batch is POLY-MAJOR:
 * polynomial b, index i at data[b * 2^log_n + i].
 * values[k] = sum_j coeffs[j] w^(jk), w = 1753635133440165772^(2^32 / n)
 * (gnark-plonky2-verifier/goldilocks/base.go:33-42). */
#define ZKLC_NTT_INVERSE 1u     /* inverse transform (includes the 1/n factor) */
#define ZKLC_NTT_IN_BITREV 2u   /* input is in bit-reversed order (output natural) */
#define ZKLC_NTT_OUT_BITREV 4u  /* leave the output in bit-reversed order (skips the permutation pass) */
/* In-place batched NTT.  coset_shift != 0 (forward, natural-order input only):
 * coefficient j is first multiplied by coset_shift^j (= evaluation on shift*<w>). */
int32_t zklc_gl_ntt(zklc_ctx *ctx, uint64_t *data, uint32_t log_n, uint32_t batch, uint32_t flags, uint64_t coset_shift);
int32_t zklc_gl_ntt_dev(zklc_ctx *ctx, void *stream, uint64_t *d_data, uint32_t log_n, uint32_t batch, uint32_t flags,
                        uint64_t coset_shift);
/* Low-degree extension: coeffs (batch x 2^log_n, natural order) -> evaluations on
 * coset_shift * <w_N>, N = 2^(log_n + rate_bits), out = batch x N; flags: ZKLC_NTT_OUT_BITREV
 * gives the order plonky2 commits to (leaf i = evaluation at shift * w^bitrev(i)). */
int32_t zklc_gl_lde(zklc_ctx *ctx, const uint64_t *coeffs, uint32_t log_n, uint32_t rate_bits, uint32_t batch,
                    uint64_t coset_shift, uint64_t *out, uint32_t flags);
int32_t zklc_gl_lde_dev(zklc_ctx *ctx, void *stream, const uint64_t *d_coeffs, uint32_t log_n, uint32_t rate_bits,
                        uint32_t batch, uint64_t coset_shift, uint64_t *d_out, uint32_t flags);
/* Poseidon-Goldilocks permutation of n states of 12 elements, in place
 * (gnark-plonky2-verifier/poseidon/goldilocks.go:30-37). */
int32_t zklc_poseidon_gl_permute(zklc_ctx *ctx, uint64_t *states, uint32_t n);
int32_t zklc_poseidon_gl_permute_dev(zklc_ctx *ctx, void *stream, uint64_t *d_states, uint32_t n);
/* Merkle tree with cap (plonky2 `MerkleTree::new`; verification side restated in
 * gnark-plonky2-verifier/fri/fri.go:97-144).  Leaf i = (mat[p * stride + i])_{p < width},
 * leaf digest = hash_or_noop, inner node = two_to_one.  tree receives all digest levels,
 * leaves first: level l (2^(log_leaves - l) digests of 4 u64) at word offset
 * sum_{j<l} 4 * 2^(log_leaves - j); the last level (l = log_leaves - cap_height) is the cap.
 * zklc_gl_merkle_tree_words gives the total size in u64 words. */
uint64_t zklc_gl_merkle_tree_words(uint32_t log_leaves, uint32_t cap_height);
int32_t zklc_gl_merkle_commit(zklc_ctx *ctx, const uint64_t *mat, uint64_t stride, uint32_t log_leaves, uint32_t width,
                              uint32_t cap_height, uint64_t *tree_out);
int32_t zklc_gl_merkle_commit_dev(zklc_ctx *ctx, void *stream, const uint64_t *d_mat, uint64_t stride, uint32_t log_leaves,
                                  uint32_t width, uint32_t cap_height, uint64_t *d_tree);

/* Poseidon-BN254 (iden3 t = 4) hasher of the last recursion -- replaces
 * crypto/plonky2_bn128/src/poseidon_bn128.rs:18-108 (`permution`) and the `Hasher` impl
 * crypto/plonky2_bn128/src/config.rs:132-199 (hash_no_pad / hash_or_noop / two_to_one).
 * states: n x 4 Fr, each 4 little-endian u64 in REGULAR (non-Montgomery) canonical form
 * (= ff's `to_repr`).  The Merkle entry points take the same poly-major Goldilocks matrix as
 * zklc_gl_merkle_commit and produce a tree of the same shape whose digests are the 32-byte
 * little-endian Fr value (= PoseidonBN128HashOut::to_bytes). */
int32_t zklc_poseidon_bn254_permute(zklc_ctx *ctx, uint64_t *states, uint32_t n);
int32_t zklc_poseidon_bn254_permute_dev(zklc_ctx *ctx, void *stream, uint64_t *d_states, uint32_t n);
int32_t zklc_bn254_merkle_commit(zklc_ctx *ctx, const uint64_t *mat, uint64_t stride, uint32_t log_leaves, uint32_t width,
                                 uint32_t cap_height, uint64_t *tree_out);
int32_t zklc_bn254_merkle_commit_dev(zklc_ctx *ctx, void *stream, const uint64_t *d_mat, uint64_t stride, uint32_t log_leaves,
                                     uint32_t width, uint32_t cap_height, uint64_t *d_tree);

/* ---- (b') plonky2 prover -------------------------------------------------------
 * Replaces `CircuitData::prove` of the un-vendored plonky2 fork (plonky2-near@2244a9d `plonk/prover.rs`
 * prove_with_partition_witness: wires commit, Z / partial products, quotient, openings, FRI), reached from
 *   near_bft_finality/src/prove_crypto/ed25519.rs:60,100 (ed25519 proofs, 2^17 rows x 234 wires)
 *   near_bft_finality/src/prove_crypto/recursion.rs:95   (recursion proofs, 2^12 rows x 135 wires)
 *   near_bft_finality/src/bin/prove_block.rs:279-287     (final wrap, Poseidon-BN128 hasher)
 * The boundary is the one of `prove_with_partition_witness`: the caller has built the circuit (gates, constants,
 * copy permutation) and generated the full witness; the library returns the proof in the byte format of
 * `ProofWithPublicInputs::to_bytes()` (what prove_block.rs:320-458 writes to proof.bin).
 * Gate constraints are evaluated by device code for the gate types in `zklc_plonky2_gate_type`
 * (the .go files of gnark-plonky2-verifier/plonk/gates and the .rs files of crypto/plonky2_u32/src/gates). */
enum zklc_plonky2_gate_type {
    ZKLC_GATE_NOOP = 0, ZKLC_GATE_CONSTANT /* p0 = num_consts */, ZKLC_GATE_PUBLIC_INPUT, ZKLC_GATE_ARITHMETIC /* p0 = num_ops */,
    ZKLC_GATE_ARITHMETIC_EXT /* p0 = num_ops */, ZKLC_GATE_MUL_EXT /* p0 = num_ops */, ZKLC_GATE_BASE_SUM /* p0 = num_limbs, p1 = base */,
    ZKLC_GATE_POSEIDON, ZKLC_GATE_POSEIDON_MDS, ZKLC_GATE_RANDOM_ACCESS /* p0 = bits, p1 = num_copies, p2 = num_extra_constants */,
    ZKLC_GATE_REDUCING /* p0 = num_coeffs */, ZKLC_GATE_REDUCING_EXT /* p0 = num_coeffs */, ZKLC_GATE_EXPONENTIATION /* p0 = num_power_bits */,
    ZKLC_GATE_COSET_INTERPOLATION /* p0 = subgroup_bits, p1 = degree; extra = weights then subgroup points */,
    ZKLC_GATE_U32_ARITHMETIC /* p0 = num_ops */, ZKLC_GATE_U32_ADD_MANY /* p0 = num_addends, p1 = num_ops */,
    ZKLC_GATE_U32_SUBTRACTION /* p0 = num_ops */, ZKLC_GATE_U32_RANGE_CHECK /* p0 = num_input_limbs */,
    ZKLC_GATE_COMPARISON /* p0 = num_bits, p1 = num_chunks */,
    /* crypto/plonky2_u32/src/gates/{interleave_u32,uninterleave_to_u32,uninterleave_to_b32}.rs (SHA-256 circuits); p0 = num_ops */
    ZKLC_GATE_U32_INTERLEAVE, ZKLC_GATE_UNINTERLEAVE_TO_U32, ZKLC_GATE_UNINTERLEAVE_TO_B32
};
typedef struct {
    uint32_t type;            /* zklc_plonky2_gate_type */
    uint32_t p[4];            /* gate parameters (see the enum) */
    uint32_t selector_index;  /* which selector polynomial filters this gate (common_data selectors_info) */
    uint32_t group_start, group_end; /* the selector group [start, end) this gate belongs to */
    uint32_t extra_off;       /* offset in u64 words into gate_extra */
} zklc_plonky2_gate;
#define ZKLC_HASHER_POSEIDON_GL 0u     /* PoseidonGoldilocksConfig (inner proofs) */
#define ZKLC_HASHER_POSEIDON_BN128 1u  /* PoseidonBN128GoldilocksConfig (final wrap, crypto/plonky2_bn128/src/config.rs:21-28) */
typedef struct {
    uint32_t degree_bits, num_wires, num_routed_wires, num_constants /* selectors included */, num_selectors, num_challenges;
    uint32_t rate_bits, cap_height, proof_of_work_bits, num_query_rounds;
    uint32_t quotient_degree_factor, num_partial_products, num_gate_constraints, num_public_inputs;
    uint32_t hasher, num_gates, num_arities, arity_bits[8];
} zklc_plonky2_params;
typedef struct zklc_plonky2_circuit zklc_plonky2_circuit;
/* gates: the circuit's gate list in common_data order (row i of the list = selector value i).  k_is: num_routed_wires
 * coset shifts.  constants: num_constants x 2^degree_bits values (poly-major, selectors first); sigmas: num_routed_wires x
 * 2^degree_bits values of the sigma polynomials on the subgroup.  All host pointers.  Preprocesses the circuit on the GPU
 * (constants_sigmas commitment, circuit digest) and allocates the prover's working set in HBM. */
int32_t zklc_plonky2_circuit_create(zklc_ctx *ctx, const zklc_plonky2_params *params, const zklc_plonky2_gate *gates,
                                    const uint64_t *gate_extra, uint32_t gate_extra_words, const uint64_t *k_is,
                                    const uint64_t *constants, const uint64_t *sigmas, zklc_plonky2_circuit **out);
void zklc_plonky2_circuit_destroy(zklc_plonky2_circuit *c);
/* verifier_only data: constants_sigmas_cap (2^cap_height digests of 32 bytes) and circuit_digest (32 bytes);
 * Goldilocks digests = 4 u64 LE, BN128 digests = the Fr value little-endian (PoseidonBN128HashOut::to_bytes) */
int32_t zklc_plonky2_verifier_data(zklc_plonky2_circuit *c, uint8_t *cap_out, uint8_t *digest_out);
uint64_t zklc_plonky2_proof_bytes(zklc_plonky2_circuit *c);
/* wires: num_wires x 2^degree_bits witness values (poly-major), public_inputs: num_public_inputs values (host).
 * proof_out receives zklc_plonky2_proof_bytes() bytes.  Returns ZKLC_ERR_INVALID_ARG when the witness does not
 * satisfy the copy constraints (the permutation product does not close). */
int32_t zklc_plonky2_prove(zklc_ctx *ctx, zklc_plonky2_circuit *c, const uint64_t *wires, const uint64_t *public_inputs,
                           uint8_t *proof_out, uint64_t proof_cap, uint64_t *proof_len);
/* same with the witness matrix already resident in HBM; work is enqueued on `stream` and the call returns when the
 * proof bytes are on the host (the Fiat-Shamir transcript runs on the host between kernels) */
int32_t zklc_plonky2_prove_dev(zklc_ctx *ctx, void *stream, zklc_plonky2_circuit *c, const uint64_t *d_wires,
                               const uint64_t *public_inputs, uint8_t *proof_out, uint64_t proof_cap, uint64_t *proof_len);
/* challenges of the last proof, for stage-by-stage parity tests: betas, gammas, alphas (num_challenges each), zeta (2),
 * fri_alpha (2), then one extension element per FRI reduction; returns the number of u64 written */
uint32_t zklc_plonky2_last_challenges(zklc_plonky2_circuit *c, uint64_t *out, uint32_t cap);
/* wall-clock milliseconds of the stages of the last proof: wires commit, partial products + commit, quotient + commit,
 * openings, FRI (combine + commit phase), PoW, queries + serialisation, total; returns the number of doubles written */
uint32_t zklc_plonky2_last_timings(zklc_plonky2_circuit *c, double *out_ms, uint32_t cap);
/* PoseidonGate witness rows (host function, no GPU): inputs n x 12, swap n (0/1, NULL = all 0) -> rows n x 135
 * in the wire layout of gnark-plonky2-verifier/plonk/gates/poseidon_gate.go:27-82 */
int32_t zklc_poseidon_gl_gate_rows(const uint64_t *inputs, const uint64_t *swap, uint32_t n, uint64_t *rows);
/* out[i] = a[i] * b[i] in the Goldilocks field (host function; canonical inputs): the circuit builder's sigma values */
void zklc_gl_mul_vec(const uint64_t *a, const uint64_t *b, uint64_t *out, uint64_t n);
/* copy classes of a circuit under construction (host function): union-find over n_pairs `connect(a, b)` records given as dense
 * target indices; root_out[i] = the smallest index of i's class.  The native part of the host circuit builder (plonky2's
 * `wire_partition`, reached from every gadget of crypto/plonky2_ed25519/src/gadgets). */
int32_t zklc_host_copy_classes(const int64_t *ia, const int64_t *ib, uint64_t n_pairs, uint64_t n_keys, int64_t *root_out);
/* Poseidon-Goldilocks parameters (gnark-plonky2-verifier/poseidon/goldilocks_constants.go): all round constants (30 x 12),
 * the optimised partial-round constants (first layer 12, one per round 22), MDS circulant + diagonal.  Used by the host
 * circuit builder to restate PoseidonGate's constraints in-circuit (recursive verifier). */
void zklc_poseidon_gl_constants(uint64_t *rc360, uint64_t *fp_first12, uint64_t *fp_rc22, uint64_t *mds_circ12, uint64_t *mds_diag12);
/* Native witness generation (host, multi-threaded; no GPU): executes the generator program of a circuit built by the host
 * builder -- the witness generators of crypto/plonky2_ed25519/src/gadgets/nonnative.rs:447-705, gadgets/curve.rs:327-370,
 * crypto/plonky2_ecdsa/src/gadgets/biguint.rs:417-470 and the gate generators of crypto/plonky2_u32/src/gates -- for
 * n_witnesses partial witnesses.  code (u32 words) = [opcode, n_params, n_in, n_out, input slots.., output slots..]*, the
 * parameters of all instructions consecutive in `params`; a slot = one copy class of the circuit
 * (zklc_amd/plonky2/builder.py `witness_program`).  wire_slot / wire_index (= col * n_rows + row): the wire cells.
 * wires_out: n_witnesses x num_wires x n_rows u64, only the circuit's wire cells are written (zero-fill once, reuse);
 * status[i] != 0 when witness i does not exist (e.g. an invalid signature: "copy constraint violated"), message in
 * err_out[200 i ..]. */
int32_t zklc_plonky2_witness_run(const uint32_t *code, uint64_t code_len, const int64_t *params, uint32_t n_slots,
                                 const uint32_t *input_slots, uint32_t n_inputs, const uint64_t *input_values, uint32_t n_witnesses,
                                 const uint32_t *wire_slot, const uint32_t *wire_index, uint64_t n_wire_entries, uint32_t num_wires,
                                 uint32_t n_rows, uint64_t *wires_out, const uint32_t *pi_slots, uint32_t n_pi, uint64_t *pi_out,
                                 int32_t *status, char *err_out, uint32_t threads);
/* the interpreter keeps its per-thread state (value arrays, one per slot) cached across calls; this frees the cache */
void zklc_plonky2_witness_release(void);

/* Witness generation ON THE GPU: the same program, levelled by data dependence and executed by the device for a
 * batch of up to 64 witnesses -- one lane per (instruction, witness), slot values stored as val[slot][witness]
 * (csrc/plonky2_witness_dev.hip).  The wire matrices are written in HBM in the prover's layout (what zklc_plonky2_prove_dev
 * takes), so the 490 MB per Ed25519 signature never cross PCIe and no host core is on the per-signature path.
 * Replaces the generators that run inside `CircuitData::prove` at near_bft_finality/src/prove_crypto/ed25519.rs:60,100 and
 * recursion.rs:95 (crypto/plonky2_ed25519/src/gadgets/nonnative.rs:447-705, gadgets/curve.rs:327-370, ...).
 * program_create copies and schedules the program once per circuit (arguments as for zklc_plonky2_witness_run);
 * run_dev: input_values host n_witnesses x n_inputs; d_wires DEVICE n_witnesses x num_wires x n_rows (only the circuit's wire
 * cells are written: zero-fill the buffer once); pi_out / status / err_out (optional, 200 bytes per witness) are host arrays,
 * valid on return (the call synchronises `stream`).  status[i] != 0: witness i does not exist (invalid signature, ...). */
typedef struct zklc_witness_program zklc_witness_program;
int32_t zklc_plonky2_witness_program_create(zklc_ctx *ctx, const uint32_t *code, uint64_t code_len, const int64_t *params,
                                            uint64_t n_params, uint32_t n_slots, const uint32_t *input_slots, uint32_t n_inputs,
                                            const uint32_t *wire_slot, const uint32_t *wire_index, uint64_t n_wire_entries,
                                            uint32_t num_wires, uint32_t n_rows, const uint32_t *pi_slots, uint32_t n_pi,
                                            zklc_witness_program **out);
void zklc_plonky2_witness_program_destroy(zklc_witness_program *p);
/* instructions, dependence levels, and the kernel launches a batch of n_witnesses takes (runs of small levels share a launch) */
int32_t zklc_plonky2_witness_program_info(zklc_witness_program *p, uint32_t n_witnesses, uint64_t *n_instr, uint32_t *n_levels,
                                          uint32_t *n_launches);
int32_t zklc_plonky2_witness_run_dev(zklc_ctx *ctx, void *stream, zklc_witness_program *p, const uint64_t *input_values,
                                     uint32_t n_witnesses, uint64_t *d_wires, uint64_t *pi_out, int32_t *status, char *err_out);

/* ---- (b'') circuit container: the hand-off between `builder.build()` and `data.prove(pw)` ------------------------
 * The reference builds a circuit once and proves with it many times: `get_ed25519_circuit_targets` /
 * `ed25519_proof_reuse_circuit` (near_bft_finality/src/prove_crypto/ed25519.rs:18-42 build, :44-66 prove; the call at :60),
 * `recursive_proof` (recursion.rs:36-94 build, :95 prove).  The container is that seam as a FILE: a flat little-endian list of
 * tagged sections holding exactly the arguments of zklc_plonky2_circuit_create and zklc_plonky2_witness_program_create, written
 * by whoever ran the circuit builder (a Rust shim beside plonky2's CircuitBuilder: INTEGRATION.md; this repo's Python mirror:
 * zklc_amd/plonky2/container.py) and loaded by any caller of this ABI (tests/c_abi/prove_from_file.c proves from two files and
 * nothing else).  Layout (csrc/container.cpp): 64-byte header (magic "ZKLCCIRC", version, section count, file size, table
 * checksum), one 32-byte table entry per section (tag, element size, offset, bytes, checksum), payload sections on 64-byte
 * boundaries.  The file functions are host code: they work without a GPU. */
#define ZKLC_CONTAINER_VERSION 1u
#define ZKLC_CONTAINER_VERIFY 1u      /* zklc_container_open flag: also check every section's checksum (reads the whole file) */
enum zklc_container_tag {
    ZKLC_SEC_PARAMS = 1,           /* one zklc_plonky2_params (hasher = the builder's default; create_from_container can override it) */
    ZKLC_SEC_GATES = 2,            /* zklc_plonky2_gate[num_gates] */
    ZKLC_SEC_GATE_EXTRA = 3,       /* u64[]: gate_extra (absent when no gate has a table) */
    ZKLC_SEC_K_IS = 4,             /* u64[num_routed_wires] */
    ZKLC_SEC_CONSTANTS = 5,        /* u64[num_constants x 2^degree_bits], selectors first */
    ZKLC_SEC_SIGMAS = 6,           /* u64[num_routed_wires x 2^degree_bits] */
    ZKLC_SEC_WP_DIMS = 16,         /* one zklc_witness_dims: the scalar arguments of zklc_plonky2_witness_program_create */
    ZKLC_SEC_WP_CODE = 17,         /* u32[code_len] */
    ZKLC_SEC_WP_PARAMS = 18,       /* i64[n_params] */
    ZKLC_SEC_WP_INPUT_SLOTS = 19,  /* u32[n_inputs] */
    ZKLC_SEC_WP_WIRE_SLOT = 20,    /* u32[n_wire_entries] */
    ZKLC_SEC_WP_WIRE_INDEX = 21,   /* u32[n_wire_entries] */
    ZKLC_SEC_WP_PI_SLOTS = 22,     /* u32[n_pi] */
    ZKLC_SEC_INPUT_VALUES = 32,    /* u64[n_witnesses x n_inputs]: a witness-input file (the PartialWitness of ed25519.rs:54-59 /
                                      recursion.rs:44-92 in the order of the program's inputs) */
    ZKLC_SEC_HOST_FIRST = 0x1000   /* tags from here on belong to the writer (target names, JSON notes); the library ignores them */
};
typedef struct {
    uint64_t code_len, n_params, n_wire_entries;
    uint32_t n_slots, n_inputs, num_wires, n_rows, n_pi, reserved;
} zklc_witness_dims;
typedef struct {
    uint32_t tag;         /* zklc_container_tag or a writer's own tag >= ZKLC_SEC_HOST_FIRST; one section per tag */
    uint32_t elem_bytes;  /* size of one element (the section is an array of them): 1, 4, 8 or a struct size */
    const void *data;
    uint64_t bytes;
} zklc_container_entry;
typedef struct zklc_container zklc_container;
/* writes `path` atomically (temporary file beside it + rename).  ZKLC_ERR_IO when the directory cannot be written. */
int32_t zklc_container_write(const char *path, const zklc_container_entry *entries, uint32_t n_entries);
/* the circuit of zklc_plonky2_circuit_create and -- when `dims` is not NULL -- the witness program of
 * zklc_plonky2_witness_program_create as one container; extra_entries: the writer's own sections (tags >= ZKLC_SEC_HOST_FIRST) */
int32_t zklc_plonky2_container_write(const char *path, const zklc_plonky2_params *params, const zklc_plonky2_gate *gates,
                                     const uint64_t *gate_extra, uint32_t gate_extra_words, const uint64_t *k_is,
                                     const uint64_t *constants, const uint64_t *sigmas, const zklc_witness_dims *dims,
                                     const uint32_t *code, const int64_t *wparams, const uint32_t *input_slots,
                                     const uint32_t *wire_slot, const uint32_t *wire_index, const uint32_t *pi_slots,
                                     const zklc_container_entry *extra_entries, uint32_t n_extra_entries);
/* maps the file read-only and checks header, size and section table (with ZKLC_CONTAINER_VERIFY: every section's checksum).
 * The data pointers of the entries stay valid until zklc_container_close. */
int32_t zklc_container_open(const char *path, uint32_t flags, zklc_container **out);
void zklc_container_close(zklc_container *c);
uint32_t zklc_container_count(const zklc_container *c);
int32_t zklc_container_entry_at(const zklc_container *c, uint32_t i, zklc_container_entry *out);
int32_t zklc_container_find(const zklc_container *c, uint32_t tag, zklc_container_entry *out);
/* after the circuit is on the GPU the mapped pages are dead weight: hand them back (the mapping stays valid) */
void zklc_container_release_pages(const zklc_container *c);
/* the parameter blocks of a circuit container after the consistency checks the create functions below run (either may be NULL) */
int32_t zklc_plonky2_container_params(const zklc_container *c, zklc_plonky2_params *params_out, zklc_witness_dims *dims_out);
/* zklc_plonky2_circuit_create / zklc_plonky2_witness_program_create with the arguments taken from the container's sections,
 * after checking that every section has the size the parameters imply and every index is in range (ZKLC_ERR_FORMAT otherwise).
 * hasher: ZKLC_HASHER_* or -1 = the one stored in the file.  The container may be closed as soon as the call returns. */
int32_t zklc_plonky2_circuit_create_from_container(zklc_ctx *ctx, const zklc_container *c, int32_t hasher, zklc_plonky2_circuit **out);
int32_t zklc_plonky2_witness_program_create_from_container(zklc_ctx *ctx, const zklc_container *c, zklc_witness_program **out);
/* zklc_plonky2_witness_run (host interpreter, no GPU) over the container's program */
int32_t zklc_plonky2_witness_run_from_container(const zklc_container *c, const uint64_t *input_values, uint32_t n_witnesses,
                                                uint64_t *wires_out, uint64_t *pi_out, int32_t *status, char *err_out, uint32_t threads);

/* ---- (b''') plonky2 verifier ---------------------------------------------------------------------------------------------
 * Replaces `CircuitData::verify` / `VerifierCircuitData::verify` of the un-vendored plonky2 fork, called right after `prove` at
 *   near_bft_finality/src/prove_block_data/primitives.rs:110,160 and header_bphash.rs:94 (`data.verify(proof)`),
 *   the tests of near_bft_finality/src/prove_crypto/ed25519.rs:175-202, recursion.rs:124-153, sha256.rs:211-215,
 * and the check a host owes the proofs that come back from remote workers (the NATS `OutputTask` of signatures.rs:144-274).
 * The checks and their order are those of gnark-plonky2-verifier (verifier/verifier.go, fri/fri.go, plonk/plonk.go):
 * format, proof of work, vanishing identity at zeta, then the query rounds in index order (per round: initial trees 0..3, then per
 * FRI reduction its consistency check and its Merkle opening, then the final polynomial).  A proof's status is its first failed
 * check.  The once-per-proof work (parse, transcript replay, gate constraints at zeta, reduced openings) runs on host threads;
 * zklc_plonky2_verify_batch runs the query phase of the whole batch on the GPU (Merkle openings and FRI fold chains, one lane each),
 * zklc_plonky2_verify_batch_host runs everything on the host.  Both give the same status for every proof. */
typedef struct zklc_plonky2_verifier zklc_plonky2_verifier;
#define ZKLC_PROOF_OK 0
#define ZKLC_PROOF_BAD_FORMAT 1    /* a u64 >= p (a BN128 digest >= r), wrong public-input count, a sibling count that contradicts common data */
#define ZKLC_PROOF_BAD_POW 2       /* the proof-of-work response has more than 64 - proof_of_work_bits bits */
#define ZKLC_PROOF_BAD_VANISHING 3 /* vanishing(zeta) != Z_H(zeta) * t(zeta) for some challenge */
#define ZKLC_PROOF_BAD_MERKLE 4    /* an initial-tree or commit-phase opening does not reach its cap */
#define ZKLC_PROOF_BAD_FRI 5       /* fold consistency or final-polynomial mismatch */
/* The circuit's common data (params, gates, gate_extra, k_is: the arguments of zklc_plonky2_circuit_create) and its verifier_only
 * data: cap = 2^min(cap_height, degree_bits + rate_bits) digests of 32 bytes, digest = 32 bytes (the zklc_plonky2_verifier_data
 * layout).  ctx may be NULL (the GPU buffers are made by the first zklc_plonky2_verify_batch; a verifier stays on that GPU).
 * ZKLC_ERR_INVALID_ARG for parameters no proof can have or an unknown gate type.  Lookups and zero-knowledge (hiding) circuits are
 * not supported: the parameters carry neither, so the caller refuses them (zklc_amd.plonky2.verifier does). */
int32_t zklc_plonky2_verifier_create(zklc_ctx *ctx, const zklc_plonky2_params *params, const zklc_plonky2_gate *gates,
                                     const uint64_t *gate_extra, uint32_t gate_extra_words, const uint64_t *k_is,
                                     const uint8_t *cap, const uint8_t *digest, zklc_plonky2_verifier **out);
/* the same for a circuit of zklc_plonky2_circuit_create: its creation arguments, and cap and digest from its commitment
 * (replaces `data.verifier_data()` + `VerifierCircuitData` of the reference's call sites) */
int32_t zklc_plonky2_verifier_create_from_circuit(zklc_ctx *ctx, zklc_plonky2_circuit *c, zklc_plonky2_verifier **out);
void zklc_plonky2_verifier_destroy(zklc_plonky2_verifier *v);
/* == zklc_plonky2_proof_bytes of the circuit */
uint64_t zklc_plonky2_verifier_proof_bytes(const zklc_plonky2_verifier *v);
/* n proofs of this circuit, each zklc_plonky2_verifier_proof_bytes long, concatenated (ProofWithPublicInputs::to_bytes()).
 * status_out[i] = ZKLC_PROOF_* of proof i.  The return value is the status of the CALL (arguments, HIP, OOM); a rejected proof is
 * not an error of the call.  The device buffers are the verifier's and only grow; host pointers, returns when the verdicts are in.
 * One call at a time per verifier (its buffers are shared state): threads that verify concurrently use one verifier each. */
int32_t zklc_plonky2_verify_batch(zklc_ctx *ctx, zklc_plonky2_verifier *v, const uint8_t *proofs, uint64_t n, int32_t *status_out);
/* the same on the host only, 1 proof per task on min(n, nthreads) threads (0 = 16) */
int32_t zklc_plonky2_verify_batch_host(zklc_plonky2_verifier *v, const uint8_t *proofs, uint64_t n, uint32_t nthreads,
                                       int32_t *status_out);
/* wall-clock milliseconds of the last zklc_plonky2_verify_batch: host stage, kernel A (Merkle openings), kernel B (FRI folds),
 * total; returns the number of doubles written */
uint32_t zklc_plonky2_verifier_last_timings(const zklc_plonky2_verifier *v, double *out_ms, uint32_t cap);

/* ---- (c) BN254---------------------------------------------------------------
 * G1 multi-scalar multiplication sum_i scalars[i] * points[i].
 * Replaces gnark-crypto `bn254.G1Affine.MultiExp` (un-vendored; gnark-plonky2-verifier/go.mod:9)
 * called from `groth16.Prove` at gnark-plonky2-verifier/cmd/web-api.go:77.
 * points: n affine points in gnark-crypto's memory layout = x then y, each 4 little-endian
 * u64 limbs in Montgomery form (x * 2^256 mod p); (0, 0) is the point at infinity.
 * scalars: n x 4 little-endian u64, REGULAR (non-Montgomery) form; expected reduced (< r) -- a scalar >= r is reduced by the
 * kernel (the points have order r), it is not an error.
 * out_affine: 8 u64 in the same layout, canonical; *out_is_infinity = 1 when the sum is
 * the point at infinity (then out_affine is zero).  Pointers must be 16-byte aligned. */
int32_t zklc_bn254_g1_msm(zklc_ctx *ctx, const uint64_t *points, const uint64_t *scalars, uint64_t n, uint64_t *out_affine,
                          uint32_t *out_is_infinity);
uint64_t zklc_bn254_g1_msm_workspace_bytes(uint64_t n);
int32_t zklc_bn254_g1_msm_dev(zklc_ctx *ctx, void *stream, const uint64_t *d_points, const uint64_t *d_scalars, uint64_t n,
                              uint64_t *d_out_affine, uint32_t *d_out_is_infinity, void *d_workspace, uint64_t workspace_bytes);

/* G2 multi-scalar multiplication (the B2 term of a Groth16 proof): replaces gnark-crypto `bn254.G2Affine.MultiExp`.
 * points: n affine G2 points = X.A0, X.A1, Y.A0, Y.A1 (4 x 4 little-endian u64, Montgomery form; all zero = infinity);
 * scalars as for the G1 MSM; out_affine: 16 u64 in the same layout. */
int32_t zklc_bn254_g2_msm(zklc_ctx *ctx, const uint64_t *points, const uint64_t *scalars, uint64_t n, uint64_t *out_affine,
                          uint32_t *out_is_infinity);
uint64_t zklc_bn254_g2_msm_workspace_bytes(uint64_t n);
int32_t zklc_bn254_g2_msm_dev(zklc_ctx *ctx, void *stream, const uint64_t *d_points, const uint64_t *d_scalars, uint64_t n,
                              uint64_t *d_out_affine, uint32_t *d_out_is_infinity, void *d_workspace, uint64_t workspace_bytes);

/* Fixed-base form of the two multi-exponentiations (round 5).  `groth16.Prove` (gnark-plonky2-verifier/cmd/web-api.go:77) multiplies
 * the SAME bases -- the proving key's pk.G1.A / pk.G1.B / pk.G1.K / pk.G1.Z and pk.G2.B -- by every proof's scalars: a table of
 * 2^(c w) * P_i for every window w (windows x n packed affine records: 64 bytes per G1 record, 128 per G2; c and the number of
 * windows are the library's choice for n and are recorded in the table's 256-byte header) is built ONCE per key, and every later
 * multi-exponentiation adds table points into one bucket set shared by all windows: no closing doublings, one bucket reduction.
 * Result: the same canonical affine point as zklc_bn254_g{1,2}_msm[_dev] on (points, scalars), bit for bit.
 *   *_table_bytes(n)   bytes of device memory the table of n bases needs;
 *   *_table_dev        builds it from n affine points in HBM (layout as for the plain form) into d_table (256-byte aligned);
 *   *_fixed_dev        the multi-exponentiation of the table's bases by d_scalars (n x 4 u64, regular form); n must be the
 *                      table's n; workspace as zklc_bn254_g{1,2}_msm_workspace_bytes(n).  ZKLC_ERR_INVALID_ARG if d_table is
 *                      not a table of this group for n bases.  Enqueue only, except a 20-byte header read. */
uint64_t zklc_bn254_g1_msm_fixed_table_bytes(uint64_t n);
int32_t zklc_bn254_g1_msm_fixed_table_dev(zklc_ctx *ctx, void *stream, const uint64_t *d_points, uint64_t n, void *d_table,
                                          uint64_t table_bytes);
int32_t zklc_bn254_g1_msm_fixed_dev(zklc_ctx *ctx, void *stream, const void *d_table, const uint64_t *d_scalars, uint64_t n,
                                    uint64_t *d_out_affine, uint32_t *d_out_is_infinity, void *d_workspace, uint64_t workspace_bytes);
uint64_t zklc_bn254_g2_msm_fixed_table_bytes(uint64_t n);
int32_t zklc_bn254_g2_msm_fixed_table_dev(zklc_ctx *ctx, void *stream, const uint64_t *d_points, uint64_t n, void *d_table,
                                          uint64_t table_bytes);
int32_t zklc_bn254_g2_msm_fixed_dev(zklc_ctx *ctx, void *stream, const void *d_table, const uint64_t *d_scalars, uint64_t n,
                                    uint64_t *d_out_affine, uint32_t *d_out_is_infinity, void *d_workspace, uint64_t workspace_bytes);

/* Pairing-product checks: is_one[b] = (prod_{i<k} e(P_{b,i}, Q_{b,i}) == 1) for `batch` independent checks.
 * Replaces gnark-crypto `bn254.PairingCheck` behind `groth16.Verify` (gnark-plonky2-verifier/cmd/web-api.go:84) and the EVM
 * pairing precompile the reference's Solidity verifier calls (contracts/hardhat/contracts/Verifier.sol:503-548: k = 4,
 * e(A,B) e(C,-delta) e(alpha,-beta) e(L_pub,-gamma)).  g1: batch x k affine G1 points (8 u64 each), g2: batch x k affine G2
 * points (16 u64 each), gnark-crypto memory layout (Montgomery); an all-zero point is the point at infinity.
 * gt_out (optional, may be NULL): the reduced pairing product of every check, 12 Fp coefficients in gnark-crypto's E12 order
 * (C0.B0.A0, C0.B0.A1, C0.B1.A0, ... C1.B2.A1), 48 u64 per check, exact exponent (p^12 - 1)/r.  Points must be on their
 * curves and in the r-torsion subgroups (as the precompile requires); this is NOT checked -- the same contract as gnark-crypto's
 * `bn254.PairingCheck`, whose caller `groth16.Verify` validates the proof's points itself (`proof.isValid()`, unchanged Go code
 * above a cgo shim); INTEGRATION.md states the precondition at the call site. */
int32_t zklc_bn254_pairing_check(zklc_ctx *ctx, const uint64_t *g1, const uint64_t *g2, uint32_t k, uint32_t batch,
                                 uint32_t *is_one, uint64_t *gt_out);
int32_t zklc_bn254_pairing_check_dev(zklc_ctx *ctx, void *stream, const uint64_t *d_g1, const uint64_t *d_g2, uint32_t k,
                                     uint32_t batch, uint32_t *d_is_one, uint64_t *d_gt_out);

/* Batched Groth16 verification, safe on untrusted proof bytes: replaces `groth16.Verify` (gnark-plonky2-verifier/cmd/web-api.go:84)
 * TOGETHER WITH the validation in front of it (`proof.isValid()`, the decoding of `proof.ReadFrom`, and the decompression at the
 * head of the contract's `verifyCompressedProof`, contracts/hardhat/contracts/Verifier.sol:427-449).  Per proof: decode, coordinates
 * reduced, A / C / B on their curves, B in the r-torsion subgroup of the twist, kSum = K[0] + sum_i x_i K[i + 1], and
 * e(A, B) e(C, -delta) e(kSum, -gamma) e(alpha, -beta) == 1.  status_out[i] is the FIRST failing class in this fixed order: */
typedef struct zklc_groth16_verifier zklc_groth16_verifier;
#define ZKLC_G16_OK 0
#define ZKLC_G16_BAD_ENCODING 1     /* a coordinate >= p; compressed form: an x >= p, or a B whose hint bit selects a root that does not exist */
#define ZKLC_G16_INFINITY 2         /* A, B or C all zero */
#define ZKLC_G16_NOT_ON_CURVE 3     /* A, then C, then B; compressed form: an x with no y */
#define ZKLC_G16_NOT_IN_SUBGROUP 4  /* B on the twist but not of order r */
#define ZKLC_G16_PAIRING 5          /* the points are valid group elements and the pairing equation does not hold */
#define ZKLC_G16_COMPRESSED 1u      /* flags: proofs are the 4 words of the contract's compressProof, not the 8 of WriteRawTo */
/* The verifying key: alpha1 (8 u64), beta2 / gamma2 / delta2 (16 u64 each), K[(n_public + 1) x 8], affine points in gnark-crypto's
 * memory layout (Montgomery limbs, as for the multi-exponentiations and the pairing entries).  The key is validated once, here:
 * coordinates reduced, on the curve, the G2 points in the r-torsion subgroup, alpha / beta / gamma / delta finite (a K point may be
 * the point at infinity); ZKLC_ERR_INVALID_ARG otherwise, and for n_public > 4096.  Also built here: the negated G2 points and a
 * fixed-base table of K[1..] (rows d 16^w K[i], 75 KiB per public input) so that the fold of a batch has no doublings.
 * ctx may be NULL (host only; the GPU buffers are made by the first zklc_groth16_verify_batch and the verifier stays on that GPU).
 * No commitment extension (the reference's key has none). */
int32_t zklc_groth16_verifier_create(zklc_ctx *ctx, const uint64_t *alpha1, const uint64_t *beta2, const uint64_t *gamma2,
                                     const uint64_t *delta2, const uint64_t *K, uint32_t n_public, zklc_groth16_verifier **out);
void zklc_groth16_verifier_destroy(zklc_groth16_verifier *v);
/* proofs: n x 256 bytes, the uncompressed encoding of `proof.WriteRawTo` (web-api.go:90-98): eight 32-byte big-endian words A.x, A.y,
 * B.x1, B.x0, B.y1, B.y0, C.x, C.y; with ZKLC_G16_COMPRESSED n x 128 bytes: A, B.c1, B.c0, C as `compressProof` writes them.
 * public_inputs: n x n_public x 4 u64, regular form; a value >= r is reduced (it is not an error).  The return value is the status
 * of the CALL (arguments, HIP, OOM; n > 2^24 is ZKLC_ERR_INVALID_ARG); a rejected proof is a status, not an error of the call.
 * Host pointers; one upload, two kernels, one read-back; returns when the verdicts are in.  The device buffers are the verifier's
 * and only grow.  One call at a time per verifier: threads that verify concurrently use one verifier each. */
int32_t zklc_groth16_verify_batch(zklc_ctx *ctx, zklc_groth16_verifier *v, const uint8_t *proofs, const uint64_t *public_inputs,
                                  uint64_t n, uint32_t flags, int32_t *status_out);
/* the same on the host only (the same lane functions compiled for the host), 1 proof per task on min(n, nthreads) threads (0 = 16) */
int32_t zklc_groth16_verify_batch_host(zklc_groth16_verifier *v, const uint8_t *proofs, const uint64_t *public_inputs, uint64_t n,
                                       uint32_t nthreads, uint32_t flags, int32_t *status_out);
/* milliseconds of the last zklc_groth16_verify_batch: upload, validation / kSum kernel, pairing kernel (device events), total (wall
 * clock); returns the number of doubles written */
uint32_t zklc_groth16_verifier_last_timings(const zklc_groth16_verifier *v, double *out_ms, uint32_t cap);

/* Batched decoding and validation of point arrays in gnark-crypto's own encoding: the A, B1, Z, K (G1) and B2 (G2) arrays of a
 * Groth16 proving key file (`pk.WriteRawTo` / `pk.WriteTo`, read back by `pk.ReadFrom`: gnark-plonky2-verifier/verifier/util.go:
 * 172-216, 337-389).  Replaces gnark-crypto `G1Affine.SetBytes` / `G2Affine.SetBytes` in the decoder's loop (ecc/bn254/marshal.go,
 * un-vendored) and establishes the precondition of the multi-exponentiations above (points on the curve), on the device.
 * bytes: n slots of fixed stride, the file's bytes as they are -- raw: G1 64 bytes X | Y, G2 128 bytes X.A1 | X.A0 | Y.A1 | Y.A0,
 * 32-byte big-endian coordinates, the two top bits of the first byte 00 (or 01: infinity); with ZKLC_POINTS_COMPRESSED: G1 32
 * bytes, G2 64 bytes, x only, top bits 10 / 11 = y is the lexicographically smaller / larger root (Fp2 ordered by A1, by A0 when
 * A1 = 0), 01 = infinity.  This is NOT the `compressProof` format of ZKLC_G16_COMPRESSED.
 * words: n x 8 (G1) / n x 16 (G2) u64, the layout the multi-exponentiations read; all zero for every point whose status is not OK.
 * status[i] (u32) is the FIRST failing class of point i in this fixed order: */
#define ZKLC_POINT_OK 0
#define ZKLC_POINT_INFINITY 1         /* a valid point, not an error: flag 01 with a zero payload, or an uncompressed (0, 0) */
#define ZKLC_POINT_BAD_ENCODING 2     /* a coordinate >= p; flag 01 with non-zero coordinate bits; a flag of the other encoding */
#define ZKLC_POINT_NOT_ON_CURVE 3     /* fails the curve equation; compressed: an x with no y */
#define ZKLC_POINT_NOT_IN_SUBGROUP 4  /* G2 with ZKLC_POINTS_CHECK_SUBGROUP: on the twist, not of order r (G1 has cofactor 1) */
#define ZKLC_POINTS_COMPRESSED 1u     /* flags */
#define ZKLC_POINTS_CHECK_SUBGROUP 2u /* G2 only */
/* summary: 4 u64 -- points OK, points at infinity, points rejected (status >= 2), index of the first rejected point (all-ones: none).
 * The *_dev entries only enqueue (one lane per point, 256 lanes per workgroup; the membership test is a second kernel over the
 * decoded words); the caller reads statuses and summary back.  d_bytes and d_words must be 16-byte aligned, n <= 2^31.  The return
 * value is the status of the CALL: ZKLC_ERR_INVALID_ARG for a misaligned or missing pointer, unknown flag bits, or
 * ZKLC_POINTS_CHECK_SUBGROUP on G1; a rejected point is a status, not an error of the call. */
int32_t zklc_bn254_g1_decode_dev(zklc_ctx *ctx, void *stream, const uint8_t *d_bytes, uint64_t n, uint32_t flags, uint64_t *d_words,
                                 uint32_t *d_status, uint64_t *d_summary);
int32_t zklc_bn254_g2_decode_dev(zklc_ctx *ctx, void *stream, const uint8_t *d_bytes, uint64_t n, uint32_t flags, uint64_t *d_words,
                                 uint32_t *d_status, uint64_t *d_summary);
/* the same on the host only (the same lane functions compiled for the host) on min(n / 256, nthreads) threads (0 = 16): host
 * pointers with the same alignment rule, no GPU and no context needed */
int32_t zklc_bn254_g1_decode_host(const uint8_t *bytes, uint64_t n, uint32_t flags, uint32_t nthreads, uint64_t *words,
                                  uint32_t *status, uint64_t *summary);
int32_t zklc_bn254_g2_decode_host(const uint8_t *bytes, uint64_t n, uint32_t flags, uint32_t nthreads, uint64_t *words,
                                  uint32_t *status, uint64_t *summary);

/* The writing direction: n points in gnark-crypto's memory layout (words: n x 8 / n x 16 u64, what the decoders above, the
 * fixed-base multiplications below and `groth16.Setup` leave) -> n slots of the encoding described above, raw or with
 * ZKLC_POINTS_COMPRESSED, exactly the bytes gnark-crypto's `RawBytes` / `Bytes` give (the point arrays `pk.WriteRawTo` / `pk.WriteTo`
 * write: util.go:172-216).  An all-zero record is the point at infinity: flag 01, zeros to the full stride.  status[i]:
 * ZKLC_POINT_OK, ZKLC_POINT_INFINITY, ZKLC_POINT_BAD_ENCODING (a coordinate's words, taken as an integer, are >= p: gnark's memory
 * form is canonical), and with ZKLC_POINTS_VALIDATE also ZKLC_POINT_NOT_ON_CURVE.  The slot of a rejected record is all 0xFF bytes,
 * which every decoder above classifies ZKLC_POINT_BAD_ENCODING.  No subgroup test: ZKLC_POINTS_CHECK_SUBGROUP is
 * ZKLC_ERR_INVALID_ARG here, as ZKLC_POINTS_VALIDATE is for the decoders.  summary, alignment (words and bytes 16 bytes), n <= 2^31
 * and the meaning of the return value are those of the decoders; the *_dev entries only enqueue (one lane per point). */
#define ZKLC_POINTS_VALIDATE 4u       /* encode only: test the curve equation */
int32_t zklc_bn254_g1_encode_dev(zklc_ctx *ctx, void *stream, const uint64_t *d_words, uint64_t n, uint32_t flags, uint8_t *d_bytes,
                                 uint32_t *d_status, uint64_t *d_summary);
int32_t zklc_bn254_g2_encode_dev(zklc_ctx *ctx, void *stream, const uint64_t *d_words, uint64_t n, uint32_t flags, uint8_t *d_bytes,
                                 uint32_t *d_status, uint64_t *d_summary);
int32_t zklc_bn254_g1_encode_host(const uint64_t *words, uint64_t n, uint32_t flags, uint32_t nthreads, uint8_t *bytes,
                                  uint32_t *status, uint64_t *summary);
int32_t zklc_bn254_g2_encode_host(const uint64_t *words, uint64_t n, uint32_t flags, uint32_t nthreads, uint8_t *bytes,
                                  uint32_t *status, uint64_t *summary);

/* NTT over the BN254 scalar field Fr.  Replaces gnark-crypto `fft.Domain.FFT / FFTInverse` (ecc/bn254/fr/fft, un-vendored)
 * inside `groth16.Prove` (gnark-plonky2-verifier/cmd/web-api.go:77).  data: 2^log_n elements in gnark-crypto's memory layout
 * (x * 2^256 mod r, 4 little-endian u64), transformed in place.  values[k] = sum_j coeffs[j] w^(jk), w = rootOfUnity^(2^28/n);
 * flags as for zklc_gl_ntt (ZKLC_NTT_INVERSE includes 1/n).  coset = 1: evaluate on / interpolate from the coset 5 * <w>
 * (gnark `fft.OnCoset()`, FrMultiplicativeGen = 5). */
int32_t zklc_bn254_fr_ntt(zklc_ctx *ctx, uint64_t *data, uint32_t log_n, uint32_t flags, uint32_t coset);
uint64_t zklc_bn254_fr_ntt_workspace_bytes(uint32_t log_n);
int32_t zklc_bn254_fr_ntt_dev(zklc_ctx *ctx, void *stream, uint64_t *d_data, uint32_t log_n, uint32_t flags, uint32_t coset,
                              void *d_workspace, uint64_t workspace_bytes);

/* d_a[i] = (d_a[i] * d_b[i] - d_c[i]) * scale over Fr (device arrays of n elements, gnark layout; scale: 4 u64, host): the
 * pointwise step of the quotient polynomial in `groth16.Prove` (gnark backend/groth16/bn254/prove.go `computeH`, un-vendored),
 * between the three coset FFTs and the coset inverse FFT; scale = 1 / (5^n - 1). */
int32_t zklc_bn254_fr_mul_sub_scale_dev(zklc_ctx *ctx, void *stream, uint64_t *d_a, const uint64_t *d_b, const uint64_t *d_c,
                                        const uint64_t *scale, uint64_t n);

/* The constraint system of `groth16.Prove(r1cs, pk, witness)` (gnark-plonky2-verifier/cmd/web-api.go:77), resident beside the
 * proving key: a = A w, b = B w, c = C w per constraint from the solved witness, straight into the buffers the transforms of
 * `computeH` take, and the test a_j b_j = c_j.  Replaces what gnark's solver leaves behind for the prover (`solution.a / b / c` of
 * constraint/bn254/solver.go, un-vendored) and its error "constraint #j is not satisfied"; SOLVING the system from the public
 * inputs (gnark's hints) and reading `r1cs.bin` stay the caller's.
 * The three matrices arrive as ONE CSR of 3 n_constraints rows: row m n_constraints + j is row j of matrix m (A, B, C = 0, 1, 2).
 * row_ptr: 3 n_constraints + 1 u64; term_wire / term_coeff: nnz u32 each, the wire and the index into coeffs; coeffs: n_coeff x 4
 * u64, gnark-crypto's memory layout (x 2^256 mod r).  No id of the dictionary has a reserved meaning.  Everything is validated
 * once, here, on the host, before anything is indexed: n_constraints <= 2^30, 1 <= n_wires <= 2^32, nnz <= 2^40, n_coeff <= 2^30
 * (sizes are compared against these bounds, never multiplied first), row_ptr[0] = 0, row_ptr non-decreasing, its last entry = nnz,
 * every wire < n_wires, every coefficient id < n_coeff, every coefficient < r; ZKLC_ERR_INVALID_ARG otherwise.  The arrays are
 * copied (the caller's may go); built here: the class of every dictionary entry (0, +1, -1, general) packed into the terms, and
 * the rows binned by length for groups of 1 / 8 / 64 lanes.  ctx may be NULL (host only: zklc_r1cs_abc_host); with a context the
 * system is uploaded to that context's GPU and zklc_r1cs_abc_dev takes contexts of that GPU. */
typedef struct zklc_r1cs zklc_r1cs;
#define ZKLC_R1CS_CHECK 1u /* flags: also test a_j b_j = c_j for j < n_constraints and fill the summary */
int32_t zklc_r1cs_create(zklc_ctx *ctx, uint64_t n_constraints, uint64_t n_wires, const uint64_t *row_ptr, const uint32_t *term_wire,
                         const uint32_t *term_coeff, uint64_t nnz, const uint64_t *coeffs, uint32_t n_coeff, zklc_r1cs **out);
void zklc_r1cs_destroy(zklc_r1cs *s);
/* bytes of device workspace one evaluation needs (the witness in Montgomery form: n_wires x 32) */
uint64_t zklc_r1cs_workspace_bytes(const zklc_r1cs *s);
/* d_witness_regular: n_wires x 4 u64, REGULAR form, the array the multi-exponentiations read as scalars (a word >= r is reduced, as
 * they do); n: the domain size, n_constraints <= n <= 2^30.  d_a, d_b, d_c: n x 4 u64 each, written in full: every element
 * canonical (< r) in gnark-crypto's Montgomery form, rows n_constraints .. n - 1 zero (the buffers need not be clear).  With
 * ZKLC_R1CS_CHECK d_summary (2 u64) receives the number of constraints with a_j b_j != c_j and the index of the first one
 * (all-ones: none); an unsatisfied system is a summary, not an error of the call.  Enqueue only: nothing is read back, the caller
 * reads the summary after the stream.  ZKLC_ERR_INVALID_ARG for n < n_constraints, a missing pointer, a witness / output /
 * workspace pointer not 16-byte aligned (summary: 8), unknown flag bits, ZKLC_R1CS_CHECK without d_summary, workspace_bytes below
 * zklc_r1cs_workspace_bytes, or a system created without a context / on another GPU. */
int32_t zklc_r1cs_abc_dev(zklc_ctx *ctx, void *stream, const zklc_r1cs *s, const uint64_t *d_witness_regular, uint64_t n,
                          uint64_t *d_a, uint64_t *d_b, uint64_t *d_c, uint32_t flags, uint64_t *d_summary, void *d_workspace,
                          uint64_t workspace_bytes);
/* the same on the host only (the same lane functions compiled for the host), 256 rows per task on up to nthreads threads (0 = 16):
 * host pointers with the same alignment rule, no GPU and no context needed; bit for bit the words and the summary of the kernels */
int32_t zklc_r1cs_abc_host(const zklc_r1cs *s, const uint64_t *witness_regular, uint64_t n, uint64_t *a, uint64_t *b, uint64_t *c,
                           uint32_t flags, uint32_t nthreads, uint64_t *summary);

/* Batched fixed-base scalar multiplication: words[i] = scalars[i] * P for one base P.  Replaces gnark-crypto
 * `bn254.BatchScalarMultiplicationG1` / `BatchScalarMultiplicationG2` (ecc/bn254/multiexp.go, un-vendored), the calls by which
 * `groth16.Setup(r1cs)` (gnark-plonky2-verifier/cmd/compile.go:40; gnark backend/groth16/bn254/setup.go) turns the scalars of a
 * key into its point arrays pk.G1.A / B / K / Z, vk.G1.K and pk.G2.B, and the single multiples alpha, beta, gamma, delta.
 * The table: ceil(254 / window_bits) rows of 2^window_bits - 1 affine points d 2^(window_bits k) P (64 bytes per G1 point, 128 per
 * G2 point: zklc_bn254_fixed_base_table_bytes; window_bits 16 = 67 / 134 MB), so that a multiple is at most one mixed addition per
 * window and no doubling.  group: ZKLC_GROUP_G1 / ZKLC_GROUP_G2.  base_words: the base in gnark-crypto's memory layout (8 / 16 u64,
 * host pointer), NULL = the generator; it must be a finite point of its curve and of order r -- the decoders above establish that,
 * it is not tested again; all-zero words (infinity), a group or a window outside 4..16 are ZKLC_ERR_INVALID_ARG.  With a context
 * the table is built by that context's GPU and stays in its memory (the call returns when it is complete); with ctx = NULL it is
 * built by host threads for the *_host entries. */
typedef struct zklc_fixed_base zklc_fixed_base;
#define ZKLC_GROUP_G1 0u
#define ZKLC_GROUP_G2 1u
int32_t zklc_bn254_fixed_base_create(zklc_ctx *ctx, uint32_t group, const uint64_t *base_words, uint32_t window_bits,
                                     zklc_fixed_base **out);
void zklc_bn254_fixed_base_destroy(zklc_fixed_base *tbl);
uint64_t zklc_bn254_fixed_base_table_bytes(uint32_t group, uint32_t window_bits);
/* bytes of device workspace a multiplication of n scalars needs (X, Y, ZZ, ZZZ and a running product per point: 200 n in G1,
 * 400 n in G2); 0 for an unknown group or n > 2^30 */
uint64_t zklc_bn254_fixed_mul_workspace_bytes(uint32_t group, uint64_t n);
/* d_scalars_regular: n x 4 u64, REGULAR form; a word >= r is reduced, as the multi-exponentiations do.  d_words: n x 8 (G1) / n x 16
 * (G2) u64, affine points in gnark-crypto's memory layout, canonical; all zero for a scalar = 0 mod r (the point at infinity, as
 * the multi-exponentiations read it).  d_summary: 2 u64 -- the number of points at infinity and the index of the first one
 * (all-ones: none).  One inversion is shared by 16 points (the workspace is where they meet).  Enqueue only: nothing is read
 * back.  ZKLC_ERR_INVALID_ARG for n > 2^30, a missing pointer, a scalar / output / workspace pointer not 16-byte aligned (summary:
 * 8), workspace_bytes below zklc_bn254_fixed_mul_workspace_bytes, a table of the other group, or one built without a context / on
 * another GPU.  The workspace holds the multiples of the caller's scalars until it is overwritten. */
int32_t zklc_bn254_g1_fixed_mul_dev(zklc_ctx *ctx, void *stream, const zklc_fixed_base *tbl, const uint64_t *d_scalars_regular,
                                    uint64_t n, uint64_t *d_words, uint64_t *d_summary, void *d_workspace, uint64_t workspace_bytes);
int32_t zklc_bn254_g2_fixed_mul_dev(zklc_ctx *ctx, void *stream, const zklc_fixed_base *tbl, const uint64_t *d_scalars_regular,
                                    uint64_t n, uint64_t *d_words, uint64_t *d_summary, void *d_workspace, uint64_t workspace_bytes);
/* the same on the host only (the same lane functions compiled for the host), 256 scalars per task on up to nthreads threads
 * (0 = 16), over a table created with ctx = NULL: host pointers with the same alignment rule; bit for bit the words and the
 * summary of the kernels.  Its own workspace is cleared before it is freed. */
int32_t zklc_bn254_g1_fixed_mul_host(const zklc_fixed_base *tbl, const uint64_t *scalars_regular, uint64_t n, uint32_t nthreads,
                                     uint64_t *words, uint64_t *summary);
int32_t zklc_bn254_g2_fixed_mul_host(const zklc_fixed_base *tbl, const uint64_t *scalars_regular, uint64_t n, uint32_t nthreads,
                                     uint64_t *words, uint64_t *summary);

/* The scalar stage of `groth16.Setup(r1cs)` (gnark-plonky2-verifier/cmd/compile.go:40; gnark backend/groth16/bn254/setup.go
 * `setupABC` and the loops around it, un-vendored): from a constraint system of zklc_r1cs_create and the toxic waste to the discrete
 * logarithms of the key's points, in the form the batched fixed-base multiplication above reads.  With L_j = L_j(tau) the Lagrange
 * basis of the subgroup of size n generated by w = 5^((r - 1) / n) (gnark-crypto's fft.Domain generator):
 *   a_t[i] = sum_j A_ji L_j, b_t[i] and c_t[i] likewise, for every wire i (the columns of the three matrices);
 *   k[i]   = (beta a_t[i] + alpha b_t[i] + c_t[i]) / gamma for i <= n_public (the constant wire and the public inputs: vk.G1.K),
 *            / delta for the other wires (pk.G1.K);
 *   z[i]   = tau^i (tau^n - 1) / delta for i < n - 1 (pk.G1.Z).
 * toxic: tau, alpha, beta, gamma, delta, 5 x 4 u64, REGULAR form, a HOST pointer in both entries; a value >= r is reduced.
 * n_public: the public inputs WITHOUT the constant wire.  n: the domain size, a power of two, max(2, n_constraints) <= n <= 2^28.
 * a_t, b_t, k: n_wires x 4 u64 each; z: (n - 1) x 4 u64; REGULAR form, canonical (< r), written in full.  A wire that occurs in no
 * A (B) column has a_t (b_t) = 0: its key point is the point at infinity.  Every stored value is exact field arithmetic made
 * canonical, so device, host threads and plain integers agree bit for bit whatever the order of a column's terms.
 * ZKLC_ERR_INVALID_ARG for gamma or delta = 0 mod r, n not a power of two or outside its range, n_public + 1 > n_wires, more than
 * 2^30 wires (what the point stage takes), a missing pointer, an output or workspace pointer not 16-byte aligned (toxic: 8),
 * workspace_bytes below zklc_groth16_setup_workspace_bytes (0 for sizes it refuses), or a system created without a context / on
 * another GPU; nothing is launched or written then.
 * The device entry transposes the system on the GPU into the workspace (a counting sort of the terms by (matrix, wire); nothing is
 * kept in the handle: a key is set up once), takes the Lagrange values as the inverse transform of (1, tau, .., tau^(n-1)), and
 * sums columns by 1 / 8 / 64 lanes, longer ones than 2048 terms by a wave per segment.  It waits ONCE on its stream, for the sizes
 * of the column lists, and returns with the rest enqueued.  The workspace holds functions of the toxic waste (tau's powers, the
 * Lagrange values, c_t) until the caller clears it; its first five u64 are the plan: columns summed by 1, 8, 64 lanes, columns cut
 * into segments, segments -- what zklc_groth16_setup_plan computes on the host from the system alone (out5: 5 u64). */
uint64_t zklc_groth16_setup_workspace_bytes(const zklc_r1cs *s, uint64_t n);
int32_t zklc_groth16_setup_scalars_dev(zklc_ctx *ctx, void *stream, const zklc_r1cs *s, const uint64_t *toxic, uint32_t n_public,
                                       uint64_t n, uint64_t *d_a_t, uint64_t *d_b_t, uint64_t *d_k, uint64_t *d_z, void *d_workspace,
                                       uint64_t workspace_bytes);
/* the same on the host only (the same lane functions compiled for the host; the Lagrange values by the quotient formula with one
 * inversion per 256), 256 lanes per task on up to nthreads threads (0 = 16): host pointers with the same alignment rule, no GPU and
 * no context needed; bit for bit the words of the kernels.  Every buffer and every named temporary that held a function of the toxic
 * waste is overwritten before the call returns (what the compiler keeps in registers or spills inside one field operation is not
 * reachable from C++ and is not claimed).  toxic is read word by word in both entries: 8-byte alignment is all it needs. */
int32_t zklc_groth16_setup_scalars_host(const zklc_r1cs *s, const uint64_t *toxic, uint32_t n_public, uint64_t n, uint32_t nthreads,
                                        uint64_t *a_t, uint64_t *b_t, uint64_t *k, uint64_t *z);
int32_t zklc_groth16_setup_plan(const zklc_r1cs *s, uint64_t *out5);
/* milliseconds between device events around the stages of the calling thread's last zklc_groth16_setup_scalars_dev: transposition
 * (with the call's one wait), powers and z, Lagrange values, column sums, combination; waits for that call's work; returns the
 * number of doubles written (0: no call of this thread has completed its launches).  The six events belong to the calling thread:
 * every zklc_groth16_setup_scalars_dev records them on its stream (a setup runs once per key; six records are nothing beside it),
 * they are created by a thread's first call, replaced when the thread moves to another GPU, and live as long as the thread's
 * runtime does -- the library has no per-thread teardown and does not destroy them. */
uint32_t zklc_groth16_setup_last_timings(double *out_ms, uint32_t cap);

#ifdef __cplusplus
}
#endif
#endif /* ZKLC_H */
