/* PC_AMGX: a native scalar algebraic multigrid behind the reference's PCCreateAMGX (pc.c:160-235, 279-295), with the
 * configuration the reference sketches at krylov.c:413-437 (AGGREGATION, SIZE_2, MULTICOLOR_DILU, V(0,3), omega 0.75,
 * DENSE_LU_SOLVER on >= 32 rows).  Kernels: csrc/k_amgx.hip.  Algorithm, and why the coarsest solve tolerates a singular
 * matrix: DESIGN.md "PC_AMGX".
 *
 * Structure (aggregates, Galerkin patterns and lists, colourings) is built on the host ONCE, in PCCreateAMGX, from the
 * values the matrix holds then -- as AMGX_solver_setup does in the reference's create -- and again only by PCAMGXRebuild.
 * PCSetup recomputes every value on the device from the current fine values: Galerkin sums in list order, the smoother's
 * diagonal, the dense LU of the coarsest level.  Levels with more than `tail_rows` rows run one launch per colour and
 * triangular pass; all smaller levels and the coarse solve run in one launch of one workgroup (setup and cycle alike).
 *
 * Options: NULL (the reference configuration), an inline AMGX string "config_version=2, key=value, ..." or the path of a
 * file holding that string or AMGX's JSON form.  The AMG parameters come from the preconditioner scope
 * (solver:preconditioner:*, JSON "preconditioner") when there is one, else from the top-level solver scope; outer-solver
 * keys (solver=FGMRES, tolerance, gmres_n_restart, ...) are ignored -- the Krylov object governs those. */
#include <ctype.h>
#include <math.h>
#include <stdarg.h>
#include <string.h>
#include "dedflow.h"
#include "dedflow_kernels.h"
#include "host_private.h"

/* ============================== options ================================================ */
#define AMGX_MAX_PAIRS 512
#define AMGX_STR 160
typedef struct AmgxPair {
    char path[AMGX_STR]; /* scope components and key, ':'-separated, "(name)" annotations removed */
    char val[AMGX_STR];
} AmgxPair;
typedef struct AmgxPairs {
    int n;
    AmgxPair p[AMGX_MAX_PAIRS];
    char pre_name[AMGX_STR]; /* "solver:preconditioner(amg)=AMG" names the preconditioner scope "amg" */
} AmgxPairs;

static void amgx_trim(char* s) {
    size_t n = strlen(s), a = 0;
    while (a < n && isspace((unsigned char)s[a])) ++a;
    while (n > a && isspace((unsigned char)s[n - 1])) --n;
    memmove(s, s + a, n - a);
    s[n - a] = '\0';
}
static void amgx_strip_quotes(char* s) {
    size_t n = strlen(s);
    if (n >= 2 && ((s[0] == '"' && s[n - 1] == '"') || (s[0] == '\'' && s[n - 1] == '\''))) {
        memmove(s, s + 1, n - 2);
        s[n - 2] = '\0';
    }
}
static int amgx_add(AmgxPairs* P, const char* path, const char* val) {
    if (P->n >= AMGX_MAX_PAIRS || strlen(path) >= AMGX_STR || strlen(val) >= AMGX_STR) return -1;
    /* "(name)" annotations: "preconditioner(amg)" names the preconditioner scope */
    char clean[AMGX_STR];
    size_t o = 0;
    for (const char* c = path; *c;) {
        if (*c == '(') {
            const char* e = strchr(c, ')');
            if (!e) return -1;
            if (o >= strlen("preconditioner") && strncmp(clean + o - strlen("preconditioner"), "preconditioner", 14) == 0 &&
                (size_t)(e - c - 1) < AMGX_STR) {
                memcpy(P->pre_name, c + 1, (size_t)(e - c - 1));
                P->pre_name[e - c - 1] = '\0';
            }
            c = e + 1;
            continue;
        }
        clean[o++] = *c++;
    }
    clean[o] = '\0';
    strcpy(P->p[P->n].path, clean);
    strcpy(P->p[P->n].val, val);
    amgx_trim(P->p[P->n].path);
    amgx_trim(P->p[P->n].val);
    amgx_strip_quotes(P->p[P->n].val);
    P->n++;
    return 0;
}

/* "key=value, key=value, ..." */
static int amgx_parse_inline(const char* text, AmgxPairs* P) {
    const char* s = text;
    while (*s) {
        const char* e = strchr(s, ',');
        size_t len = e ? (size_t)(e - s) : strlen(s);
        char tok[2 * AMGX_STR];
        if (len >= sizeof tok) return -1;
        memcpy(tok, s, len);
        tok[len] = '\0';
        amgx_trim(tok);
        if (tok[0]) {
            char* eq = strchr(tok, '=');
            if (!eq) return -1;
            *eq = '\0';
            if (amgx_add(P, tok, eq + 1)) return -1;
        }
        if (!e) break;
        s = e + 1;
    }
    return 0;
}

/* minimal JSON: objects, strings, numbers (and true / false / null as words); nested objects become path components */
typedef struct { const char* s; } JsonCur;
static void js_ws(JsonCur* c) { while (*c->s && isspace((unsigned char)*c->s)) c->s++; }
static int js_string(JsonCur* c, char* out, size_t cap) {
    if (*c->s != '"') return -1;
    c->s++;
    size_t o = 0;
    while (*c->s && *c->s != '"') {
        char ch = *c->s++;
        if (ch == '\\' && *c->s) ch = *c->s++;
        if (o + 1 >= cap) return -1;
        out[o++] = ch;
    }
    if (*c->s != '"') return -1;
    c->s++;
    out[o] = '\0';
    return 0;
}
static int js_object(JsonCur* c, const char* prefix, AmgxPairs* P, int depth) {
    if (depth > 16) return -1;
    js_ws(c);
    if (*c->s != '{') return -1;
    c->s++;
    js_ws(c);
    if (*c->s == '}') { c->s++; return 0; }
    for (;;) {
        char key[AMGX_STR], path[AMGX_STR];
        js_ws(c);
        if (js_string(c, key, sizeof key)) return -1;
        js_ws(c);
        if (*c->s != ':') return -1;
        c->s++;
        js_ws(c);
        if (snprintf(path, sizeof path, "%s%s%s", prefix, prefix[0] ? ":" : "", key) >= (int)sizeof path) return -1;
        if (*c->s == '{') {
            if (js_object(c, path, P, depth + 1)) return -1;
        } else {
            char val[AMGX_STR];
            if (*c->s == '"') {
                if (js_string(c, val, sizeof val)) return -1;
            } else {
                size_t o = 0;
                while (*c->s && *c->s != ',' && *c->s != '}' && !isspace((unsigned char)*c->s)) {
                    if (o + 1 >= sizeof val) return -1;
                    val[o++] = *c->s++;
                }
                val[o] = '\0';
                if (!o) return -1;
            }
            if (amgx_add(P, path, val)) return -1;
        }
        js_ws(c);
        if (*c->s == ',') { c->s++; continue; }
        if (*c->s == '}') { c->s++; return 0; }
        return -1;
    }
}

static int amgx_in(const char* name, const char* const* list) {
    for (int i = 0; list[i]; ++i)
        if (strcmp(name, list[i]) == 0) return 1;
    return 0;
}
static int amgx_err(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    fprintf(stderr, "PCCreateAMGX: ");
    vfprintf(stderr, fmt, ap);
    fprintf(stderr, "\n");
    va_end(ap);
    return -1;
}
static int amgx_int(const char* key, const char* v, int lo, int32_t* out) {
    char* end;
    long x = strtol(v, &end, 10);
    if (end == v || *end || x < lo || x > 1000000) return amgx_err("%s=%s: expected an integer >= %d", key, v, lo);
    *out = (int32_t)x;
    return 0;
}

static void amgx_defaults(DflAMGXConfig* c) { /* krylov.c:413-437 */
    memset(c, 0, sizeof *c);
    c->relaxation_factor = 0.75;
    c->selector_passes = 1;
    c->smoother = DFL_AMGX_SMOOTHER_DILU;
    c->presweeps = 0;
    c->postsweeps = 3;
    c->max_levels = 100;
    c->min_coarse_rows = 32;
    c->max_iters = 1;
}

int DflAMGXParseConfig(const char* options, DflAMGXConfig* cfg) {
    amgx_defaults(cfg);
    if (!options) return 0;
    /* a readable file holds the configuration; anything else is the configuration itself */
    char* text = NULL;
    FILE* f = fopen(options, "rb");
    if (f) {
        fseek(f, 0, SEEK_END);
        long len = ftell(f);
        fseek(f, 0, SEEK_SET);
        if (len < 0 || len > (1 << 20)) { fclose(f); return amgx_err("%s: unreadable or too large", options); }
        text = (char*)malloc((size_t)len + 1);
        size_t got = fread(text, 1, (size_t)len, f);
        text[got] = '\0';
        fclose(f);
    } else {
        text = strdup(options);
    }
    AmgxPairs* P = (AmgxPairs*)calloc(1, sizeof(AmgxPairs));
    const char* t = text;
    while (*t && isspace((unsigned char)*t)) ++t;
    int rc;
    if (*t == '{') {
        JsonCur c = {t};
        rc = js_object(&c, "", P, 0);
        js_ws(&c);
        if (!rc && *c.s) rc = -1;
    } else {
        /* a file may spread the inline form over lines */
        for (char* q = text; *q; ++q)
            if (*q == '\n' || *q == '\r') *q = ' ';
        rc = amgx_parse_inline(t, P);
    }
    free(text);
    if (rc) {
        free(P);
        return amgx_err("cannot parse the configuration");
    }
    /* scope of every pair: preconditioner (a "preconditioner" component, or the named preconditioner scope) or top */
    static const char* const amg_keys[] = {"algorithm", "selector", "smoother", "presweeps", "postsweeps", "relaxation_factor",
                                           "max_levels", "min_coarse_rows", "coarse_solver", "cycle", "max_iters", "solver", NULL};
    static const char* const ignored[] = {"config_version", "scope", "monitor_residual", "convergence", "tolerance", "norm",
                                          "print_solve_stats", "print_grid_stats", "obtain_timings", "use_scalar_norm",
                                          "gmres_n_restart", "error_scaling", "max_uncolored_percentage",
                                          "matrix_coloring_scheme", "store_res_history", "print_config", "determinism_flag",
                                          "exception_handling", "print_vis_data", "preconditioner", NULL};
    int scope[AMGX_MAX_PAIRS];
    int has_pre = 0;
    for (int i = 0; i < P->n; ++i) {
        char tmp[AMGX_STR];
        strcpy(tmp, P->p[i].path);
        char* last = strrchr(tmp, ':');
        scope[i] = 0;
        if (last) {
            *last = '\0';
            for (char* tok = strtok(tmp, ":"); tok; tok = strtok(NULL, ":")) {
                amgx_trim(tok);
                if (strcmp(tok, "preconditioner") == 0 || (P->pre_name[0] && strcmp(tok, P->pre_name) == 0)) scope[i] = 1;
            }
        }
        has_pre |= scope[i];
    }
    char unknown[1024] = "";
    rc = 0;
    for (int i = 0; i < P->n && !rc; ++i) {
        const char* key = strrchr(P->p[i].path, ':');
        key = key ? key + 1 : P->p[i].path;
        const char* v = P->p[i].val;
        const int amg_scope = has_pre ? scope[i] == 1 : 1;
        if (amgx_in(key, ignored)) continue;
        if (!amgx_in(key, amg_keys)) {
            cfg->unknown_keys++;
            if (strlen(unknown) + strlen(P->p[i].path) + 3 < sizeof unknown) {
                if (unknown[0]) strcat(unknown, ", ");
                strcat(unknown, P->p[i].path);
            }
            continue;
        }
        if (!amg_scope) continue; /* the outer solver's keys: the Krylov object governs those */
        if (strcmp(key, "solver") == 0) {
            if (has_pre && strcmp(v, "AMG") != 0) rc = amgx_err("solver=%s: only AMG is supported as the preconditioner", v);
        } else if (strcmp(key, "algorithm") == 0) {
            if (strcmp(v, "AGGREGATION") != 0) rc = amgx_err("algorithm=%s: only AGGREGATION is supported", v);
        } else if (strcmp(key, "selector") == 0) {
            if (strcmp(v, "SIZE_2") == 0) cfg->selector_passes = 1;
            else if (strcmp(v, "SIZE_4") == 0) cfg->selector_passes = 2;
            else if (strcmp(v, "SIZE_8") == 0) cfg->selector_passes = 3;
            else rc = amgx_err("selector=%s: supported are SIZE_2, SIZE_4, SIZE_8", v);
        } else if (strcmp(key, "smoother") == 0) {
            if (strcmp(v, "MULTICOLOR_DILU") == 0) cfg->smoother = DFL_AMGX_SMOOTHER_DILU;
            else if (strcmp(v, "BLOCK_JACOBI") == 0) cfg->smoother = DFL_AMGX_SMOOTHER_JACOBI;
            else rc = amgx_err("smoother=%s: supported are MULTICOLOR_DILU, BLOCK_JACOBI", v);
        } else if (strcmp(key, "coarse_solver") == 0) {
            if (strcmp(v, "DENSE_LU_SOLVER") != 0) rc = amgx_err("coarse_solver=%s: only DENSE_LU_SOLVER is supported", v);
        } else if (strcmp(key, "cycle") == 0) {
            if (strcmp(v, "V") != 0) rc = amgx_err("cycle=%s: only V is supported", v);
        } else if (strcmp(key, "relaxation_factor") == 0) {
            char* end;
            double x = strtod(v, &end);
            if (end == v || *end || !(x > 0.0) || !isfinite(x)) rc = amgx_err("relaxation_factor=%s: expected a positive number", v);
            else cfg->relaxation_factor = x;
        } else if (strcmp(key, "presweeps") == 0) rc = amgx_int(key, v, 0, &cfg->presweeps);
        else if (strcmp(key, "postsweeps") == 0) rc = amgx_int(key, v, 0, &cfg->postsweeps);
        else if (strcmp(key, "max_levels") == 0) rc = amgx_int(key, v, 1, &cfg->max_levels);
        else if (strcmp(key, "min_coarse_rows") == 0) rc = amgx_int(key, v, 1, &cfg->min_coarse_rows);
        else if (strcmp(key, "max_iters") == 0) rc = amgx_int(key, v, 1, &cfg->max_iters);
    }
    if (unknown[0]) fprintf(stderr, "PCCreateAMGX: ignoring unknown option keys: %s\n", unknown);
    free(P);
    return rc;
}

/* ============================== hierarchy (host) ======================================= */
/* position of column j in row i (columns ascending), -1 if not stored */
static index_type amgx_find(const index_type* rp, const index_type* ci, index_type i, index_type j) {
    index_type lo = rp[i], hi = rp[i + 1] - 1;
    while (lo <= hi) {
        const index_type mid = lo + (hi - lo) / 2;
        if (ci[mid] == j) return mid;
        if (ci[mid] < j) lo = mid + 1;
        else hi = mid - 1;
    }
    return -1;
}

/* one pairwise pass.  Strength w_ij = (|a_ij|/|a_ii| + |a_ji|/|a_jj|) / 2 (a_ji = 0 if not stored; a ratio with a zero
 * diagonal counts 0); only neighbours with w_ij > 0 count.  Four handshake rounds: every unaggregated row picks its
 * strongest unaggregated neighbour (ties: the smaller column), mutual picks become pairs.  A row left over joins the
 * aggregate of its strongest neighbour if the rounds paired that one, else it stays a singleton.  Aggregates are numbered
 * in the order of their smallest member.  Returns the number of aggregates. */
static index_type amgx_pairwise(index_type n, const index_type* rp, const index_type* ci, const f64* val, index_type* agg) {
    const index_type nnz = rp[n];
    f64* dg = (f64*)malloc(sizeof(f64) * (size_t)(n > 0 ? n : 1));
    f64* w = (f64*)malloc(sizeof(f64) * (size_t)(nnz > 0 ? nnz : 1));
    index_type* label = (index_type*)malloc(sizeof(index_type) * (size_t)(n > 0 ? n : 1));
    index_type* pick = (index_type*)malloc(sizeof(index_type) * (size_t)(n > 0 ? n : 1));
    for (index_type i = 0; i < n; ++i) {
        const index_type d = amgx_find(rp, ci, i, i);
        dg[i] = d >= 0 ? fabs(val[d]) : 0.0;
    }
    for (index_type i = 0; i < n; ++i)
        for (index_type k = rp[i]; k < rp[i + 1]; ++k) {
            const index_type j = ci[k];
            if (j == i) { w[k] = 0.0; continue; }
            const index_type t = amgx_find(rp, ci, j, i);
            const f64 aij = dg[i] > 0.0 ? fabs(val[k]) / dg[i] : 0.0;
            const f64 aji = (t >= 0 && dg[j] > 0.0) ? fabs(val[t]) / dg[j] : 0.0;
            w[k] = 0.5 * (aij + aji);
        }
    for (index_type i = 0; i < n; ++i) label[i] = -1;
    for (int round = 0; round < 4; ++round) {
        for (index_type i = 0; i < n; ++i) {
            pick[i] = -1;
            if (label[i] >= 0) continue;
            f64 best = 0.0;
            for (index_type k = rp[i]; k < rp[i + 1]; ++k) {
                const index_type j = ci[k];
                if (j == i || label[j] >= 0) continue;
                if (w[k] > best) { best = w[k]; pick[i] = j; } /* ascending columns: the smaller j wins a tie */
            }
        }
        for (index_type i = 0; i < n; ++i) {
            const index_type j = pick[i];
            if (j > i && pick[j] == i) label[i] = label[j] = i;
        }
    }
    /* leftovers: decided against the paired state of the rounds only, so the order does not matter */
    for (index_type i = 0; i < n; ++i) {
        pick[i] = -1;
        if (label[i] >= 0) continue;
        f64 best = 0.0;
        index_type s = -1;
        for (index_type k = rp[i]; k < rp[i + 1]; ++k)
            if (ci[k] != i && w[k] > best) { best = w[k]; s = ci[k]; }
        pick[i] = s;
    }
    for (index_type i = 0; i < n; ++i)
        if (label[i] < 0) {
            const index_type s = pick[i];
            label[i] = (s >= 0 && label[s] >= 0) ? label[s] : -2 - i; /* -2 - i: singleton, resolved below */
        }
    for (index_type i = 0; i < n; ++i)
        if (label[i] <= -2) label[i] = i;
    /* numbering by the smallest member (pick reused as the smallest member of each label) */
    for (index_type i = 0; i < n; ++i) pick[i] = n;
    for (index_type i = 0; i < n; ++i)
        if (i < pick[label[i]]) pick[label[i]] = i;
    index_type nc = 0;
    index_type* id = (index_type*)malloc(sizeof(index_type) * (size_t)(n > 0 ? n : 1));
    for (index_type i = 0; i < n; ++i)
        if (pick[label[i]] == i) id[label[i]] = nc++;
    for (index_type i = 0; i < n; ++i) agg[i] = id[label[i]];
    free(id);
    free(dg);
    free(w);
    free(label);
    free(pick);
    return nc;
}

/* Galerkin structure of P^T A P for the map agg (nc aggregates): coarse pattern (columns ascending), per coarse nonzero the
 * ascending list of fine nonzeros summed into it, and (if val) the coarse values in that order */
typedef struct AmgxGal {
    index_type nc, nnz;
    index_type *rp, *ci, *goff, *gidx;
    f64* val;
} AmgxGal;
static void amgx_galerkin_host(index_type n, const index_type* rp, const index_type* ci, const f64* val, const index_type* agg,
                               index_type nc, AmgxGal* G) {
    index_type* aoff = (index_type*)calloc((size_t)nc + 1, sizeof(index_type));
    index_type* amem = (index_type*)malloc(sizeof(index_type) * (size_t)(n > 0 ? n : 1));
    for (index_type i = 0; i < n; ++i) aoff[agg[i] + 1]++;
    for (index_type c = 0; c < nc; ++c) aoff[c + 1] += aoff[c];
    index_type* cur = (index_type*)malloc(sizeof(index_type) * (size_t)(nc + 1));
    memcpy(cur, aoff, sizeof(index_type) * (size_t)nc);
    for (index_type i = 0; i < n; ++i) amem[cur[agg[i]]++] = i;
    index_type* mark = (index_type*)malloc(sizeof(index_type) * (size_t)(nc > 0 ? nc : 1));
    for (index_type c = 0; c < nc; ++c) mark[c] = -1;
    G->nc = nc;
    G->rp = (index_type*)calloc((size_t)nc + 1, sizeof(index_type));
    size_t cap = (size_t)rp[n] + 1, used = 0;
    G->ci = (index_type*)malloc(sizeof(index_type) * cap);
    for (index_type c = 0; c < nc; ++c) {
        const size_t start = used;
        for (index_type t = aoff[c]; t < aoff[c + 1]; ++t) {
            const index_type i = amem[t];
            for (index_type k = rp[i]; k < rp[i + 1]; ++k) {
                const index_type J = agg[ci[k]];
                if (mark[J] != c) { mark[J] = c; G->ci[used++] = J; }
            }
        }
        /* insertion sort of the row (short rows) */
        for (size_t a = start + 1; a < used; ++a) {
            const index_type v = G->ci[a];
            size_t b = a;
            while (b > start && G->ci[b - 1] > v) { G->ci[b] = G->ci[b - 1]; --b; }
            G->ci[b] = v;
        }
        G->rp[c + 1] = (index_type)used;
    }
    G->nnz = (index_type)used;
    const index_type nnzf = rp[n];
    index_type* pos = (index_type*)malloc(sizeof(index_type) * (size_t)(nnzf > 0 ? nnzf : 1));
    G->goff = (index_type*)calloc((size_t)G->nnz + 1, sizeof(index_type));
    for (index_type i = 0; i < n; ++i)
        for (index_type k = rp[i]; k < rp[i + 1]; ++k) {
            pos[k] = amgx_find(G->rp, G->ci, agg[i], agg[ci[k]]);
            G->goff[pos[k] + 1]++;
        }
    for (index_type k = 0; k < G->nnz; ++k) G->goff[k + 1] += G->goff[k];
    G->gidx = (index_type*)malloc(sizeof(index_type) * (size_t)(nnzf > 0 ? nnzf : 1));
    index_type* fill = (index_type*)malloc(sizeof(index_type) * (size_t)(G->nnz > 0 ? G->nnz : 1));
    memcpy(fill, G->goff, sizeof(index_type) * (size_t)G->nnz);
    for (index_type k = 0; k < nnzf; ++k) G->gidx[fill[pos[k]]++] = k;
    G->val = NULL;
    if (val) {
        G->val = (f64*)malloc(sizeof(f64) * (size_t)(G->nnz > 0 ? G->nnz : 1));
        for (index_type k = 0; k < G->nnz; ++k) {
            f64 s = 0.0;
            for (index_type t = G->goff[k]; t < G->goff[k + 1]; ++t) s += val[G->gidx[t]];
            G->val[k] = s;
        }
    }
    free(fill);
    free(pos);
    free(mark);
    free(cur);
    free(aoff);
    free(amem);
}
static void amgx_gal_free(AmgxGal* G) {
    free(G->rp);
    free(G->ci);
    free(G->goff);
    free(G->gidx);
    free(G->val);
    memset(G, 0, sizeof *G);
}

/* `passes` pairwise passes composed (SIZE_2 / 4 / 8), each later one on the Galerkin graph of the previous */
static index_type amgx_aggregate(index_type n, const index_type* rp, const index_type* ci, const f64* val, int passes,
                                 index_type* agg) {
    index_type nc = amgx_pairwise(n, rp, ci, val, agg);
    AmgxGal G = {0};
    const index_type *crp = rp, *cci = ci;
    const f64* cval = val;
    index_type cn = n;
    index_type* a2 = NULL;
    for (int p = 1; p < passes && nc > 1; ++p) {
        AmgxGal H = {0};
        amgx_galerkin_host(cn, crp, cci, cval, p == 1 ? agg : a2, nc, &H);
        if (p > 1) amgx_gal_free(&G);
        G = H;
        /* the map of this pass applies to the previous coarse rows; compose (a2 keeps it for the next Galerkin graph) */
        if (p == 1) a2 = (index_type*)malloc(sizeof(index_type) * (size_t)(nc > 0 ? nc : 1));
        index_type* step = (index_type*)malloc(sizeof(index_type) * (size_t)(nc > 0 ? nc : 1));
        const index_type nc2 = amgx_pairwise(nc, G.rp, G.ci, G.val, step);
        for (index_type i = 0; i < n; ++i) agg[i] = step[agg[i]];
        memcpy(a2, step, sizeof(index_type) * (size_t)nc);
        free(step);
        cn = nc;
        crp = G.rp;
        cci = G.ci;
        cval = G.val;
        nc = nc2;
    }
    if (passes > 1) amgx_gal_free(&G);
    free(a2);
    return nc;
}

index_type DflAMGXAggregateHost(index_type n, const index_type* rp, const index_type* ci, const f64* val, int passes,
                                index_type* agg_out) {
    return amgx_aggregate(n, rp, ci, val, passes < 1 ? 1 : passes, agg_out);
}

/* greedy colouring in ascending row order: the smallest colour no already-coloured neighbour has */
static index_type amgx_color(index_type n, const index_type* rp, const index_type* ci, index_type* color) {
    index_type* mark = (index_type*)malloc(sizeof(index_type) * (size_t)(n + 1));
    for (index_type c = 0; c <= n; ++c) mark[c] = -1;
    index_type nc = 0;
    for (index_type i = 0; i < n; ++i) color[i] = -1;
    for (index_type i = 0; i < n; ++i) {
        for (index_type k = rp[i]; k < rp[i + 1]; ++k) {
            const index_type j = ci[k];
            if (j != i && color[j] >= 0) mark[color[j]] = i;
        }
        index_type c = 0;
        while (mark[c] == i) ++c;
        color[i] = c;
        if (c + 1 > nc) nc = c + 1;
    }
    free(mark);
    return nc;
}

/* ============================== the preconditioner ===================================== */
#define AMGX_MAX_COARSE 2048 /* rows of the coarsest level: the dense LU runs in one workgroup */

typedef struct AmgxLevel {
    dfl_amgx_level d;      /* device pointers as the kernels see them */
    index_type* coff;      /* host [ncolor+1] */
    CSRAttr attr;          /* the level's pattern (device row_ptr / col_ind) for PCAMGXLevelMatrix */
    Matrix* mat;           /* CSR view of the level's values */
    b32 own_val;           /* val allocated here (not the caller's CSR values) */
} AmgxLevel;

typedef struct PCAmgx {
    DflAMGXConfig cfg;
    Matrix* A;              /* MAT_TYPE_CSR with its own values, or a view of a block-mode MatrixFS */
    const value_type* block_val; /* view: the parent's 4x4 blocks (entry [3][3] is A11) */
    index_type nlev, l0;    /* levels; the first level of the tail */
    index_type tail_rows;
    AmgxLevel* lev;
    dfl_amgx_level* d_lev;  /* device copy of the level records (the tail kernels read it) */
    b32 d_lev_stale;        /* the records changed since they were copied */
    value_type *t0, *e0, *w1; /* level 0: residual of later cycles, their correction, a second scratch */
    int64_t launches_apply, launches_setup;
    f64 op_complexity;
} PCAmgx;

static void* amgx_dev(size_t bytes) { return CdamMallocDevice((ptrdiff_t)(bytes > 0 ? bytes : 8)); }
static void* amgx_up(const void* h, size_t bytes) {
    void* d = amgx_dev(bytes);
    if (bytes) HIPGUARD(hipMemcpy(d, h, bytes, H2D));
    return d;
}

static void amgx_free_levels(PCAmgx* p) {
    if (!p->lev) return;
    HIPGUARD(hipStreamSynchronize(DflStream()));
    for (index_type l = 0; l < p->nlev; ++l) {
        AmgxLevel* L = &p->lev[l];
        dfl_amgx_level* d = &L->d;
        if (L->mat) {
            ((MatrixCSR*)L->mat->data)->val = NULL; /* the values belong to this object or to the caller */
            MatrixDestroy(L->mat);
        }
        void* ptrs[] = {(void*)d->rp, (void*)d->ci, (void*)d->diag, (void*)d->trans, (void*)d->color, (void*)d->rows,
                        (void*)d->coff, (void*)d->agg, (void*)d->aoff, (void*)d->amem, (void*)d->goff, (void*)d->gidx,
                        d->einv, d->b, d->x, d->w, d->lu, d->piv};
        for (size_t k = 0; k < sizeof ptrs / sizeof ptrs[0]; ++k)
            if (ptrs[k]) CdamFreeDevice(ptrs[k], 0);
        if (L->own_val) CdamFreeDevice(d->val, 0);
        free(L->coff);
    }
    free(p->lev);
    p->lev = NULL;
    if (p->d_lev) CdamFreeDevice(p->d_lev, 0);
    if (p->t0) CdamFreeDevice(p->t0, 0);
    if (p->e0) CdamFreeDevice(p->e0, 0);
    if (p->w1) CdamFreeDevice(p->w1, 0);
    p->d_lev = NULL;
    p->t0 = p->e0 = p->w1 = NULL;
    p->nlev = 0;
}

/* the fine matrix: pattern and current values on the host; FALSE if it is not a supported kind */
static b32 amgx_fine(PCAmgx* p, index_type* n_out, const CSRAttr** attr_out, value_type** dval_out) {
    Matrix* A = p->A;
    if (!A || A->type != MAT_TYPE_CSR) return FALSE;
    MatrixCSR* c = (MatrixCSR*)A->data;
    const CSRAttr* at = c->attr;
    if (!at || at->num_row != at->num_col || at->parent) return FALSE; /* scalar, square, not row-expanded */
    p->block_val = NULL;
    if (c->owner && c->owner->block_mode) {
        MatrixFS* fs = c->owner;
        if (c->owner_slot != fs->n_offset + 1 || fs->spy1x1 != at || fs->owned_rows != at->num_row) return FALSE;
        p->block_val = fs->block_val;
        *dval_out = NULL;
    } else {
        if (!c->val) return FALSE;
        *dval_out = c->val;
    }
    *n_out = at->num_row;
    *attr_out = at;
    return TRUE;
}

static void amgx_level_matrix(AmgxLevel* L) {
    L->attr.num_row = L->attr.num_col = L->d.n;
    L->attr.nnz = L->d.nnz;
    L->attr.row_ptr = (index_type*)L->d.rp;
    L->attr.col_ind = (index_type*)L->d.ci;
    L->attr.parent = NULL;
    L->mat = MatrixCreateTypeCSR(&L->attr, NULL);
    ((MatrixCSR*)L->mat->data)->val = L->d.val;
}

/* structure of every level; returns FALSE (with a message) if the hierarchy cannot be built */
static b32 amgx_build(PCAmgx* p) {
    index_type n;
    const CSRAttr* at;
    value_type* dval;
    if (!amgx_fine(p, &n, &at, &dval)) {
        fprintf(stderr, "PCCreateAMGX: needs a square MAT_TYPE_CSR matrix with its own values or the A11 view of a block-mode "
                        "MatrixFS on one GPU\n");
        return FALSE;
    }
    hipStream_t s = DflStream();
    HIPGUARD(hipStreamSynchronize(s));
    index_type* rp = (index_type*)malloc(sizeof(index_type) * ((size_t)n + 1));
    HIPGUARD(hipMemcpy(rp, at->row_ptr, sizeof(index_type) * ((size_t)n + 1), D2H));
    const index_type nnz = rp[n];
    index_type* ci = (index_type*)malloc(sizeof(index_type) * (size_t)(nnz > 0 ? nnz : 1));
    f64* val = (f64*)malloc(sizeof(f64) * (size_t)(nnz > 0 ? nnz : 1));
    HIPGUARD(hipMemcpy(ci, at->col_ind, sizeof(index_type) * (size_t)nnz, D2H));
    value_type* v0 = dval;
    if (p->block_val) {
        v0 = (value_type*)amgx_dev(sizeof(f64) * (size_t)nnz);
        dfl_amgx_gather_a11(nnz, p->block_val, v0, s);
    }
    HIPGUARD(hipMemcpy(val, v0, sizeof(f64) * (size_t)nnz, D2H));
    b32 ok = TRUE;
    for (index_type i = 0; i < n && ok; ++i) {
        for (index_type k = rp[i] + 1; k < rp[i + 1]; ++k)
            if (ci[k] <= ci[k - 1]) ok = FALSE;
        if (amgx_find(rp, ci, i, i) < 0) ok = FALSE;
    }
    if (!ok) {
        fprintf(stderr, "PCCreateAMGX: every row needs its diagonal and ascending column indices\n");
        if (p->block_val) CdamFreeDevice(v0, 0);
        free(rp);
        free(ci);
        free(val);
        return FALSE;
    }
    /* levels: host arrays of the current level, coarsened until a stop rule holds */
    int cap = 8;
    p->lev = (AmgxLevel*)calloc((size_t)cap, sizeof(AmgxLevel));
    p->nlev = 0;
    index_type *crp = rp, *cci = ci, cn = n;
    f64* cval = val;
    index_type* goff = NULL;
    index_type* gidx = NULL;
    f64 nnz_total = 0.0;
    for (;;) {
        if (p->nlev == cap) {
            cap *= 2;
            p->lev = (AmgxLevel*)realloc(p->lev, sizeof(AmgxLevel) * (size_t)cap);
            memset(p->lev + cap / 2, 0, sizeof(AmgxLevel) * (size_t)(cap / 2));
        }
        AmgxLevel* L = &p->lev[p->nlev++];
        dfl_amgx_level* d = &L->d;
        const index_type cnnz = crp[cn];
        nnz_total += cnnz;
        d->n = cn;
        d->nnz = cnnz;
        d->rp = (index_type*)amgx_up(crp, sizeof(index_type) * ((size_t)cn + 1));
        d->ci = (index_type*)amgx_up(cci, sizeof(index_type) * (size_t)cnnz);
        if (p->nlev == 1) {
            d->val = v0;
            L->own_val = p->block_val != NULL;
        } else {
            d->val = (value_type*)amgx_up(cval, sizeof(f64) * (size_t)cnnz);
            L->own_val = TRUE;
            d->goff = (index_type*)amgx_up(goff, sizeof(index_type) * ((size_t)cnnz + 1));
            d->gidx = (index_type*)amgx_up(gidx, sizeof(index_type) * (size_t)p->lev[p->nlev - 2].d.nnz);
            free(goff);
            free(gidx);
            goff = gidx = NULL;
        }
        {
            index_type* h = (index_type*)malloc(sizeof(index_type) * (size_t)(cnnz > 0 ? cnnz : 1));
            index_type* dg = (index_type*)malloc(sizeof(index_type) * (size_t)(cn > 0 ? cn : 1));
            for (index_type i = 0; i < cn; ++i) {
                dg[i] = amgx_find(crp, cci, i, i);
                for (index_type k = crp[i]; k < crp[i + 1]; ++k) h[k] = amgx_find(crp, cci, cci[k], i);
            }
            d->trans = (index_type*)amgx_up(h, sizeof(index_type) * (size_t)cnnz);
            d->diag = (index_type*)amgx_up(dg, sizeof(index_type) * (size_t)cn);
            /* colouring, rows grouped by colour */
            index_type* color = h;
            if (cnnz < cn) color = (index_type*)realloc(h, sizeof(index_type) * (size_t)cn), h = color;
            d->ncolor = amgx_color(cn, crp, cci, color);
            L->coff = (index_type*)calloc((size_t)d->ncolor + 1, sizeof(index_type));
            for (index_type i = 0; i < cn; ++i) L->coff[color[i] + 1]++;
            for (index_type c = 0; c < d->ncolor; ++c) L->coff[c + 1] += L->coff[c];
            index_type* cur = (index_type*)malloc(sizeof(index_type) * (size_t)(d->ncolor + 1));
            memcpy(cur, L->coff, sizeof(index_type) * (size_t)d->ncolor);
            for (index_type i = 0; i < cn; ++i) dg[cur[color[i]]++] = i;
            d->rows = (index_type*)amgx_up(dg, sizeof(index_type) * (size_t)cn);
            d->color = (index_type*)amgx_up(color, sizeof(index_type) * (size_t)cn);
            d->coff = (index_type*)amgx_up(L->coff, sizeof(index_type) * ((size_t)d->ncolor + 1));
            free(cur);
            free(h);
            free(dg);
        }
        d->einv = (value_type*)amgx_dev(sizeof(f64) * (size_t)cn);
        d->b = (value_type*)amgx_dev(sizeof(f64) * (size_t)cn);
        d->x = (value_type*)amgx_dev(sizeof(f64) * (size_t)cn);
        d->w = (value_type*)amgx_dev(sizeof(f64) * (size_t)cn);
        /* stop rules: small enough, level budget, a pass that keeps more than 90 % of the rows */
        b32 last = cn <= p->cfg.min_coarse_rows || p->nlev >= p->cfg.max_levels;
        index_type* agg = NULL;
        index_type nc = 0;
        if (!last) {
            agg = (index_type*)malloc(sizeof(index_type) * (size_t)(cn > 0 ? cn : 1));
            nc = amgx_aggregate(cn, crp, cci, cval, p->cfg.selector_passes, agg);
            if ((f64)nc > 0.9 * (f64)cn) last = TRUE;
        }
        if (last) {
            free(agg);
            if (cn > AMGX_MAX_COARSE) {
                fprintf(stderr, "PCCreateAMGX: the coarsest level keeps %d rows (more than %d): no hierarchy\n", cn, AMGX_MAX_COARSE);
                ok = FALSE;
            } else {
                d->lu = (value_type*)amgx_dev(sizeof(f64) * (size_t)cn * (size_t)cn);
                d->piv = (index_type*)amgx_dev(sizeof(index_type) * 2 * (size_t)cn);
                d->zpiv = d->piv + cn;
            }
            break;
        }
        AmgxGal G = {0};
        amgx_galerkin_host(cn, crp, cci, cval, agg, nc, &G);
        {
            index_type* aoff = (index_type*)calloc((size_t)nc + 1, sizeof(index_type));
            index_type* amem = (index_type*)malloc(sizeof(index_type) * (size_t)(cn > 0 ? cn : 1));
            for (index_type i = 0; i < cn; ++i) aoff[agg[i] + 1]++;
            for (index_type c = 0; c < nc; ++c) aoff[c + 1] += aoff[c];
            index_type* cur = (index_type*)malloc(sizeof(index_type) * (size_t)(nc + 1));
            memcpy(cur, aoff, sizeof(index_type) * (size_t)nc);
            for (index_type i = 0; i < cn; ++i) amem[cur[agg[i]]++] = i;
            d->nc = nc;
            d->agg = (index_type*)amgx_up(agg, sizeof(index_type) * (size_t)cn);
            d->aoff = (index_type*)amgx_up(aoff, sizeof(index_type) * ((size_t)nc + 1));
            d->amem = (index_type*)amgx_up(amem, sizeof(index_type) * (size_t)cn);
            free(aoff);
            free(amem);
            free(cur);
        }
        free(agg);
        if (crp != rp) { free(crp); free(cci); free(cval); }
        crp = G.rp;
        cci = G.ci;
        cval = G.val;
        goff = G.goff;
        gidx = G.gidx;
        cn = nc;
    }
    if (crp != rp) { free(crp); free(cci); free(cval); }
    free(goff);
    free(gidx);
    free(rp);
    free(ci);
    free(val);
    if (!ok) {
        amgx_free_levels(p);
        return FALSE;
    }
    p->op_complexity = nnz > 0 ? nnz_total / (f64)nnz : 1.0;
    /* the tail: the first level with at most tail_rows rows, the coarsest at the latest */
    p->l0 = p->nlev - 1;
    for (index_type l = 0; l < p->nlev; ++l)
        if (p->lev[l].d.n <= p->tail_rows) { p->l0 = l; break; }
    for (index_type l = 0; l < p->nlev; ++l) amgx_level_matrix(&p->lev[l]);
    p->t0 = (value_type*)amgx_dev(sizeof(f64) * (size_t)n);
    p->e0 = (value_type*)amgx_dev(sizeof(f64) * (size_t)n);
    p->w1 = (value_type*)amgx_dev(sizeof(f64) * (size_t)n);
    p->d_lev = (dfl_amgx_level*)amgx_dev(sizeof(dfl_amgx_level) * (size_t)p->nlev);
    p->d_lev_stale = TRUE;
    return TRUE;
}

static void amgx_upload_levels(PCAmgx* p) {
    dfl_amgx_level* h = (dfl_amgx_level*)malloc(sizeof(dfl_amgx_level) * (size_t)p->nlev);
    for (index_type l = 0; l < p->nlev; ++l) h[l] = p->lev[l].d;
    HIPGUARD(hipMemcpy(p->d_lev, h, sizeof(dfl_amgx_level) * (size_t)p->nlev, H2D));
    free(h);
}

static void amgx_setup(PC* pc) {
    PCAmgx* p = (PCAmgx*)pc->data;
    hipStream_t s = DflStream();
    int64_t nl = 0;
    AmgxLevel* L0 = &p->lev[0];
    MatrixCSR* c = (MatrixCSR*)p->A->data;
    if (p->block_val) {
        p->block_val = c->owner->block_val; /* the parent may have moved its block array (placement calibration) */
        dfl_amgx_gather_a11(L0->d.nnz, p->block_val, L0->d.val, s);
        nl++;
    } else if (c->val != L0->d.val) {
        L0->d.val = c->val;
        ((MatrixCSR*)L0->mat->data)->val = c->val;
        p->d_lev_stale = TRUE;
    }
    if (p->d_lev_stale) {
        amgx_upload_levels(p);
        p->d_lev_stale = FALSE;
    }
    const b32 jac = p->cfg.smoother == DFL_AMGX_SMOOTHER_JACOBI;
    for (index_type l = 0; l < p->l0; ++l) {
        AmgxLevel* L = &p->lev[l];
        if (l >= 1) { dfl_amgx_galerkin(L->d, p->lev[l - 1].d.val, s); nl++; }
        if (jac) { dfl_amgx_jacobi_setup(L->d, s); nl++; }
        else
            for (index_type cc = 0; cc < L->d.ncolor; ++cc) {
                dfl_amgx_dilu_setup_color(L->d, cc, L->coff[cc], L->coff[cc + 1] - L->coff[cc], s);
                nl++;
            }
    }
    dfl_amgx_tail_setup(p->d_lev, p->l0, p->nlev, jac, s);
    nl++;
    p->launches_setup = nl;
}

/* one smoothing step on grid level L (x / w swapped by Jacobi) */
static int64_t amgx_smooth(PCAmgx* p, AmgxLevel* L, dfl_amgx_level* d, b32 x_zero) {
    hipStream_t s = DflStream();
    const f64 om = p->cfg.relaxation_factor;
    if (p->cfg.smoother == DFL_AMGX_SMOOTHER_JACOBI) {
        dfl_amgx_jacobi_sweep(*d, om, x_zero, s);
        value_type* t = d->x;
        d->x = d->w;
        d->w = t;
        return 1;
    }
    for (index_type c = 0; c < d->ncolor; ++c) dfl_amgx_dilu_forward(*d, c, L->coff[c], L->coff[c + 1] - L->coff[c], x_zero, s);
    for (index_type c = d->ncolor - 1; c >= 0; --c)
        dfl_amgx_dilu_backward(*d, c, L->coff[c], L->coff[c + 1] - L->coff[c], om, x_zero, s);
    return 2 * (int64_t)d->ncolor;
}

/* where a level's iterate ends after pre + post sweeps that started in x (Jacobi alternates x and w) */
static value_type* amgx_final_x(const PCAmgx* p, index_type l, value_type* x, value_type* w) {
    if (l == p->nlev - 1) return x;
    const int sweeps = p->cfg.presweeps + p->cfg.postsweeps;
    return (p->cfg.smoother == DFL_AMGX_SMOOTHER_JACOBI && (sweeps & 1)) ? w : x;
}

/* one V-cycle from a zero initial guess: b -> x (level 0 uses b / x / w given here) */
static int64_t amgx_vcycle(PCAmgx* p, const value_type* b, value_type* x, value_type* w) {
    hipStream_t s = DflStream();
    int64_t nl = 0;
    const int pre = p->cfg.presweeps, post = p->cfg.postsweeps;
    dfl_amgx_level cur[64]; /* grid levels: the records with level 0's vectors and Jacobi's x / w exchanges applied */
    ASSERT(p->l0 <= 64);
    for (index_type l = 0; l < p->l0; ++l) {
        cur[l] = p->lev[l].d;
        if (l == 0) {
            cur[0].b = (value_type*)b;
            cur[0].x = x;
            cur[0].w = w;
        }
        for (int k = 0; k < pre; ++k) nl += amgx_smooth(p, &p->lev[l], &cur[l], k == 0);
        dfl_amgx_restrict(cur[l], p->lev[l + 1].d, pre == 0, s);
        nl++;
    }
    const b32 jac = p->cfg.smoother == DFL_AMGX_SMOOTHER_JACOBI;
    if (p->l0 == 0) dfl_amgx_tail_cycle(p->d_lev, 0, p->nlev, jac, pre, post, p->cfg.relaxation_factor, b, x, w, s);
    else {
        dfl_amgx_level* t = &p->lev[p->l0].d;
        dfl_amgx_tail_cycle(p->d_lev, p->l0, p->nlev, jac, pre, post, p->cfg.relaxation_factor, t->b, t->x, t->w, s);
    }
    nl++;
    for (index_type l = p->l0 - 1; l >= 0; --l) {
        const dfl_amgx_level* C = &p->lev[l + 1].d;
        dfl_amgx_prolong(cur[l], amgx_final_x(p, l + 1, C->x, C->w), pre == 0, s);
        nl++;
        for (int k = 0; k < post; ++k) nl += amgx_smooth(p, &p->lev[l], &cur[l], FALSE);
    }
    return nl;
}

/* z = M^-1 r: max_iters V-cycles, the first from z = 0, every further one z += V(r - A z) */
static void amgx_apply(PC* pc, value_type* r, value_type* z) {
    PCAmgx* p = (PCAmgx*)pc->data;
    hipStream_t s = DflStream();
    const index_type n = p->lev[0].d.n;
    const b32 odd = p->cfg.smoother == DFL_AMGX_SMOOTHER_JACOBI && p->nlev > 1 &&
                    ((p->cfg.presweeps + p->cfg.postsweeps) & 1);
    int64_t nl = 0;
    for (int it = 0; it < p->cfg.max_iters; ++it) {
        const value_type* b = r;
        value_type* out = z;
        if (it > 0) {
            dfl_amgx_residual(p->lev[0].d, r, z, p->t0, s);
            nl++;
            b = p->t0;
            out = p->e0;
        }
        /* the cycle's iterate starts in x and ends in x or w: arrange for it to end in `out` */
        if (odd) nl += amgx_vcycle(p, b, p->w1, out);
        else nl += amgx_vcycle(p, b, out, p->w1);
        if (it > 0) {
            dfl_daxpy(n, 1.0, p->e0, z, s);
            nl++;
        }
    }
    p->launches_apply = nl;
}

static void amgx_destroy(PC* pc) {
    PCAmgx* p = (PCAmgx*)pc->data;
    amgx_free_levels(p);
    free(p);
}

PC* PCCreateAMGX(Matrix* mat, void* options) {
    DflAMGXConfig cfg;
    if (DflAMGXParseConfig((const char*)options, &cfg)) return NULL;
    PCAmgx* p = (PCAmgx*)calloc(1, sizeof(PCAmgx));
    p->cfg = cfg;
    p->A = mat;
    p->tail_rows = 8192;
    const char* e = getenv("DFL_AMGX_TAIL_ROWS");
    if (e && *e) p->tail_rows = (index_type)atoi(e);
    if (!amgx_build(p)) {
        free(p);
        return NULL;
    }
    PC* pc = (PC*)CdamMallocHost(SIZE_OF(PC));
    memset(pc, 0, sizeof *pc);
    pc->type = PC_AMGX;
    pc->mat = mat;
    pc->data = p;
    pc->op->setup = amgx_setup;
    pc->op->apply = amgx_apply;
    pc->op->destroy = amgx_destroy;
    return pc;
}

void PCAMGXRebuild(PC* pc) {
    ASSERT(pc && pc->type == PC_AMGX);
    PCAmgx* p = (PCAmgx*)pc->data;
    amgx_free_levels(p);
    if (!amgx_build(p)) ASSERT(0 && "PCAMGXRebuild: the hierarchy cannot be rebuilt from the current values");
}

static PCAmgx* amgx_of(PC* pc) {
    ASSERT(pc && pc->type == PC_AMGX);
    return (PCAmgx*)pc->data;
}
index_type PCAMGXNumLevels(PC* pc) { return amgx_of(pc)->nlev; }
void PCAMGXInfo(PC* pc, index_type* rows, index_type* nnz, index_type* colors, f64* op_complexity, index_type* tail_level,
                int64_t* launches_apply, int64_t* launches_setup) {
    PCAmgx* p = amgx_of(pc);
    for (index_type l = 0; l < p->nlev; ++l) {
        if (rows) rows[l] = p->lev[l].d.n;
        if (nnz) nnz[l] = p->lev[l].d.nnz;
        if (colors) colors[l] = p->lev[l].d.ncolor;
    }
    if (op_complexity) *op_complexity = p->op_complexity;
    if (tail_level) *tail_level = p->l0;
    if (launches_apply) *launches_apply = p->launches_apply;
    if (launches_setup) *launches_setup = p->launches_setup;
}
const index_type* PCAMGXLevelAggregates(PC* pc, index_type l) {
    PCAmgx* p = amgx_of(pc);
    return (l >= 0 && l < p->nlev) ? p->lev[l].d.agg : NULL;
}
const index_type* PCAMGXLevelColors(PC* pc, index_type l) {
    PCAmgx* p = amgx_of(pc);
    return (l >= 0 && l < p->nlev) ? p->lev[l].d.color : NULL;
}
Matrix* PCAMGXLevelMatrix(PC* pc, index_type l) {
    PCAmgx* p = amgx_of(pc);
    return (l >= 0 && l < p->nlev) ? p->lev[l].mat : NULL;
}
const index_type* PCAMGXCoarsePivots(PC* pc) {
    PCAmgx* p = amgx_of(pc);
    return p->lev[p->nlev - 1].d.piv;
}
