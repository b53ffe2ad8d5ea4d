/* Options of PC_AMGX (pc_amgx.c): NULL (the reference configuration, krylov.c:413-437), an inline AMGX string
 * "config_version=2, key=value, ..." or the path of a file holding that string or AMGX's JSON form.  The AMG parameters come
 * from the preconditioner scope (solver:preconditioner:*, JSON "preconditioner") when there is one, else from the top-level
 * solver scope; outer-solver keys (solver=FGMRES, tolerance, gmres_n_restart, ...) are ignored -- the Krylov object governs
 * those.  Every key the parser acts on is one row of amgx_opts[]; a key without a row is reported and ignored. */
#include <ctype.h>
#include <math.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "dedflow.h"

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

/* One row per key.  OPT_INT: an integer >= lo into the int32 at `target`; OPT_REAL: a positive real into the f64 there;
 * OPT_WORD: one of `words`, its value into the int32 there; OPT_ONLY: must equal words[0] (nothing is stored; pre_only:
 * checked only when the configuration has a preconditioner scope -- without one, solver=... names the AMG itself). */
typedef enum { OPT_INT, OPT_REAL, OPT_WORD, OPT_ONLY } AmgxOptKind;
typedef struct AmgxWord {
    const char* word;
    int32_t value;
} AmgxWord;
typedef struct AmgxOpt {
    const char* key;
    AmgxOptKind kind;
    size_t target;
    int lo;
    AmgxWord words[4]; /* ends at a NULL word */
    int pre_only;
} AmgxOpt;
#define CFG(field) offsetof(DflAMGXConfig, field)
static const AmgxOpt amgx_opts[] = {
    {"solver", OPT_ONLY, 0, 0, {{"AMG", 0}}, 1},
    {"algorithm", OPT_ONLY, 0, 0, {{"AGGREGATION", 0}}},
    {"coarse_solver", OPT_ONLY, 0, 0, {{"DENSE_LU_SOLVER", 0}}},
    {"cycle", OPT_ONLY, 0, 0, {{"V", 0}}},
    {"selector", OPT_WORD, CFG(selector_passes), 0, {{"SIZE_2", 1}, {"SIZE_4", 2}, {"SIZE_8", 3}}},
    {"smoother", OPT_WORD, CFG(smoother), 0,
     {{"MULTICOLOR_DILU", DFL_AMGX_SMOOTHER_DILU}, {"BLOCK_JACOBI", DFL_AMGX_SMOOTHER_JACOBI}}},
    {"relaxation_factor", OPT_REAL, CFG(relaxation_factor), 0},
    {"presweeps", OPT_INT, CFG(presweeps), 0},
    {"postsweeps", OPT_INT, CFG(postsweeps), 0},
    {"max_levels", OPT_INT, CFG(max_levels), 1},
    {"min_coarse_rows", OPT_INT, CFG(min_coarse_rows), 1},
    {"max_iters", OPT_INT, CFG(max_iters), 1},
};
#undef CFG
static const char* const ignored[] = {"config_version", "scope", "monitor_residual", "convergence", "tolerance", "norm",
                                      "print_solve_stats", "print_grid_stats", "obtain_timings", "use_scalar_norm",
                                      "gmres_n_restart", "error_scaling", "max_uncolored_percentage",
                                      "matrix_coloring_scheme", "store_res_history", "print_config", "determinism_flag",
                                      "exception_handling", "print_vis_data", "preconditioner", NULL};

static const AmgxOpt* amgx_opt(const char* key) {
    for (size_t i = 0; i < sizeof amgx_opts / sizeof amgx_opts[0]; ++i)
        if (strcmp(key, amgx_opts[i].key) == 0) return &amgx_opts[i];
    return NULL;
}

/* value v of option o into cfg; 0 = accepted */
static int amgx_set(const AmgxOpt* o, const char* v, int has_pre, DflAMGXConfig* cfg) {
    void* target = (char*)cfg + o->target;
    char* end;
    switch (o->kind) {
    case OPT_INT: {
        const long x = strtol(v, &end, 10);
        if (end == v || *end || x < o->lo || x > 1000000) return amgx_err("%s=%s: expected an integer >= %d", o->key, v, o->lo);
        *(int32_t*)target = (int32_t)x;
        return 0;
    }
    case OPT_REAL: {
        const double x = strtod(v, &end);
        if (end == v || *end || !(x > 0.0) || !isfinite(x)) return amgx_err("%s=%s: expected a positive number", o->key, v);
        *(f64*)target = x;
        return 0;
    }
    case OPT_WORD: {
        char list[AMGX_STR] = "";
        for (int w = 0; w < 4 && o->words[w].word; ++w) {
            if (strcmp(v, o->words[w].word) == 0) {
                *(int32_t*)target = o->words[w].value;
                return 0;
            }
            if (w) strcat(list, ", ");
            strcat(list, o->words[w].word);
        }
        return amgx_err("%s=%s: supported are %s", o->key, v, list);
    }
    case OPT_ONLY:
        if ((o->pre_only && !has_pre) || strcmp(v, o->words[0].word) == 0) return 0;
        return amgx_err("%s=%s: only %s is supported%s", o->key, v, o->words[0].word, o->pre_only ? " as the preconditioner" : "");
    }
    return -1;
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
        if (amgx_in(key, ignored)) continue;
        const AmgxOpt* o = amgx_opt(key);
        if (!o) {
            cfg->unknown_keys++;
            if (strlen(unknown) + strlen(P->p[i].path) + 3 < sizeof unknown) {
                if (unknown[0]) strcat(unknown, ", ");
                strcat(unknown, P->p[i].path);
            }
            continue;
        }
        if (has_pre && !scope[i]) continue; /* the outer solver's keys: the Krylov object governs those */
        rc = amgx_set(o, P->p[i].val, has_pre, cfg);
    }
    if (unknown[0]) fprintf(stderr, "PCCreateAMGX: ignoring unknown option keys: %s\n", unknown);
    free(P);
    return rc;
}
