/*
 * A plain-C consumer of include/cattus_hip.h that evaluates leaves the way a search thread of the reference does -- one blocking call per
 * leaf from each of T threads (engine/src/util/batch.rs:49-177), then the softmax over the leaf's legal moves
 * (calc_moves_probs, engine/src/net/mod.rs:100-119) -- in two ways, and reports what each costs:
 *
 *     mode A   cattus_hip_apply(1 leaf), then the softmax on the calling thread: all M logits cross to the host
 *     mode B   cattus_hip_apply_legal(1 leaf): the softmax runs on the device, the leaf's probabilities cross
 *
 *   consumer_legal BLOB LEAVES dtype batch_size threads plane_words rounds
 *
 * BLOB: weight blob.  LEAVES: u32 n, u32 words (u64 words per leaf), u32 total, u32 0; u64 planes [n][words]; u32 off [n + 1]; u16 idx [total]
 * (leaf i's legal moves are idx[off[i] .. off[i + 1])).  The modes alternate in one process, A B A B ..., `rounds` times each over all n
 * leaves, on one evaluator; one JSON line on stdout: per mode the leaves evaluated, leaves per second, the mean batch fill (positions per
 * batch, from cattus_hip_stats) and the bytes copied device -> host per leaf (from the sizes the two entry points copy: M logits + a value,
 * or the leaf's probabilities + a value), and the largest difference between the two modes' probabilities (they use different exps).
 * No Python, no ctypes: gcc -std=c99 consumer_legal.c -lcattus_hip -lpthread -lm.
 */
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "cattus_hip.h"

typedef struct worker {
    cattus_eval* ev;
    const uint64_t* planes;
    const uint32_t* off;
    const uint16_t* idx;
    float* probs; /* [total], at the lists' places */
    float* logits; /* this thread's [moves], mode A */
    uint32_t first, stride, n, words, moves;
    int mode_b, rc;
    char err[256];
} worker;

static void* run(void* arg) {
    worker* w = (worker*)arg;
    for (uint32_t i = w->first; i < w->n; i += w->stride) {
        const uint64_t* leaf = w->planes + (size_t)i * w->words;
        const uint16_t* list = w->idx + w->off[i];
        const uint32_t count = w->off[i + 1] - w->off[i];
        float* out = w->probs + w->off[i];
        float value;
        int rc;
        if (w->mode_b) {
            const uint32_t span[2] = {0, count};
            rc = cattus_hip_apply_legal(w->ev, leaf, 1, list, span, out, &value);
        } else {
            rc = cattus_hip_apply(w->ev, leaf, 1, w->logits, &value);
            if (rc == CATTUS_OK) { /* calc_moves_probs: max from f32::MIN, exp, the sum in move order */
                float mx = -3.40282347e+38f, sum = 0.0f;
                for (uint32_t k = 0; k < count; k++) mx = w->logits[list[k]] > mx ? w->logits[list[k]] : mx;
                for (uint32_t k = 0; k < count; k++) sum += out[k] = expf(w->logits[list[k]] - mx);
                for (uint32_t k = 0; k < count; k++) out[k] /= sum;
            }
        }
        if (rc != CATTUS_OK) {
            w->rc = rc;
            snprintf(w->err, sizeof w->err, "%s", cattus_hip_last_error()); /* thread-local message */
            return NULL;
        }
    }
    return NULL;
}

static void* slurp(const char* path, size_t* size) {
    FILE* f = fopen(path, "rb");
    if (!f) return NULL;
    fseek(f, 0, SEEK_END);
    *size = (size_t)ftell(f);
    fseek(f, 0, SEEK_SET);
    void* p = malloc(*size ? *size : 1);
    if (p && fread(p, 1, *size, f) != *size) {
        free(p);
        p = NULL;
    }
    fclose(f);
    return p;
}

static double now(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

typedef struct tally {
    uint64_t leaves, batches, positions;
    double seconds;
} tally;

int main(int argc, char** argv) {
    if (argc != 8) {
        fprintf(stderr, "usage: %s BLOB LEAVES dtype batch_size threads plane_words rounds\n", argv[0]);
        return 2;
    }
    size_t blob_size = 0, leaves_size = 0;
    void* blob = slurp(argv[1], &blob_size);
    unsigned char* file = (unsigned char*)slurp(argv[2], &leaves_size);
    if (!blob || !file || leaves_size < 16) {
        fprintf(stderr, "cannot read inputs\n");
        return 2;
    }
    uint32_t head[4];
    memcpy(head, file, sizeof head);
    const uint32_t n = head[0], words = head[1], total = head[2];
    const size_t planes_bytes = (size_t)n * words * 8, off_bytes = ((size_t)n + 1) * 4;
    if (leaves_size != 16 + planes_bytes + off_bytes + (size_t)total * 2) {
        fprintf(stderr, "leaves file: %zu bytes for n %u, words %u, total %u\n", leaves_size, n, words, total);
        return 2;
    }
    /* copies with the alignment of their element types */
    uint64_t* planes = (uint64_t*)malloc(planes_bytes ? planes_bytes : 1);
    uint32_t* off = (uint32_t*)malloc(off_bytes);
    uint16_t* idx = (uint16_t*)malloc(total ? (size_t)total * 2 : 1);
    float* probs_a = (float*)calloc(total ? total : 1, sizeof(float));
    float* probs_b = (float*)calloc(total ? total : 1, sizeof(float));
    if (!planes || !off || !idx || !probs_a || !probs_b) return 2;
    memcpy(planes, file + 16, planes_bytes);
    memcpy(off, file + 16 + planes_bytes, off_bytes);
    memcpy(idx, file + 16 + planes_bytes + off_bytes, (size_t)total * 2);
    if (off[0] != 0 || off[n] != total) {
        fprintf(stderr, "leaves file: offsets do not span the lists\n");
        return 2;
    }

    cattus_eval_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.struct_size = sizeof cfg;
    cfg.device = 0;
    cfg.dtype = (uint32_t)atoi(argv[3]);
    cfg.max_batch = (uint32_t)atoi(argv[4]);
    cfg.plane_words = (uint32_t)atoi(argv[6]);
    cfg.flush_us = 200;
    const int threads = atoi(argv[5]), rounds = atoi(argv[7]);
    if (threads < 1 || rounds < 1) return 2;

    cattus_eval* ev = NULL;
    if (cattus_hip_create(blob, blob_size, &cfg, &ev) != CATTUS_OK) {
        fprintf(stderr, "create: %s\n", cattus_hip_last_error());
        return 1;
    }
    cattus_net_desc d;
    cattus_hip_desc(ev, &d);
    if (words != d.planes * cfg.plane_words) {
        fprintf(stderr, "leaves file: %u words per leaf, the network takes %u\n", words, d.planes * cfg.plane_words);
        cattus_hip_destroy(ev);
        return 2;
    }

    pthread_t* tid = (pthread_t*)calloc((size_t)threads, sizeof *tid);
    worker* ws = (worker*)calloc((size_t)threads, sizeof *ws);
    float* logits = (float*)calloc((size_t)threads * d.moves, sizeof(float));
    tally tl[2];
    memset(tl, 0, sizeof tl);
    int failed = 0;
    for (int pass = 0; pass < 2 * rounds && !failed; pass++) {
        const int mode_b = pass & 1;
        cattus_stats s0, s1;
        cattus_hip_stats(ev, &s0);
        const double t0 = now();
        for (int t = 0; t < threads; t++) {
            memset(&ws[t], 0, sizeof ws[t]);
            ws[t].ev = ev, ws[t].planes = planes, ws[t].off = off, ws[t].idx = idx;
            ws[t].probs = mode_b ? probs_b : probs_a, ws[t].logits = logits + (size_t)t * d.moves;
            ws[t].first = (uint32_t)t, ws[t].stride = (uint32_t)threads, ws[t].n = n, ws[t].words = words, ws[t].moves = d.moves;
            ws[t].mode_b = mode_b;
            pthread_create(&tid[t], NULL, run, &ws[t]);
        }
        for (int t = 0; t < threads; t++) {
            pthread_join(tid[t], NULL);
            if (ws[t].rc) {
                fprintf(stderr, "mode %c, thread %d: %s (%d)\n", mode_b ? 'B' : 'A', t, ws[t].err, ws[t].rc);
                failed = 1;
            }
        }
        tl[mode_b].seconds += now() - t0;
        cattus_hip_stats(ev, &s1);
        tl[mode_b].leaves += n, tl[mode_b].batches += s1.batches - s0.batches, tl[mode_b].positions += s1.positions - s0.positions;
    }
    cattus_hip_destroy(ev);

    float max_diff = 0.0f;
    for (uint32_t k = 0; k < total; k++) {
        const float diff = fabsf(probs_a[k] - probs_b[k]);
        if (!(diff <= max_diff)) max_diff = diff; /* a NaN shows */
    }
    const double d2h[2] = {4.0 * d.moves + 4.0, n ? 4.0 * total / n + 4.0 : 0.0};
    printf("{\"threads\": %d, \"max_batch\": %u, \"moves\": %u, \"mean_legal\": %.2f, \"max_prob_diff\": %.3g", threads, cfg.max_batch, d.moves,
           n ? (double)total / n : 0.0, (double)max_diff);
    for (int m = 0; m < 2; m++)
        printf(", \"%c\": {\"leaves\": %llu, \"leaves_per_s\": %.1f, \"batch_fill\": %.2f, \"d2h_bytes_per_leaf\": %.1f}", m ? 'B' : 'A',
               (unsigned long long)tl[m].leaves, tl[m].seconds > 0 ? (double)tl[m].leaves / tl[m].seconds : 0.0,
               tl[m].batches ? (double)tl[m].positions / (double)tl[m].batches : 0.0, d2h[m]);
    printf("}\n");
    free(tid), free(ws), free(logits), free(blob), free(file), free(planes), free(off), free(idx), free(probs_a), free(probs_b);
    return failed;
}
