/* Plain C99 caller of libscaloam_hip.so: include/scaloam_hip.h must compile with `gcc -std=c99 -pedantic-errors` and every stage's
 * create entry point must link and fail cleanly (SCAL_E_NO_DEVICE) on a host without a gfx950 device, or succeed and be destroyed on one.
 * Prints "abi ok <version> devices=<n>"; exit code 0. */
#include <stdio.h>
#include <string.h>
#include "scaloam_hip.h"

int main(void) {
    scal_features_config fc;
    scal_features_t* f = NULL;
    scal_pipeline_config pc;
    scal_pipeline_t* p = NULL;
    scal_refine_config rc_cfg;
    scal_refine_t* rf = NULL;
    scal_reloc_config rl_cfg;
    scal_reloc_t* rl = NULL;
    scal_nbr_config nb_cfg;
    scal_nbr_t* nb = NULL;
    int rc, n = scal_device_count();
    memset(&fc, 0, sizeof fc);
    fc.lidar_type = SCAL_HDL64, fc.n_scans = 64, fc.minimum_range = 5.0, fc.max_points = 1000, fc.check_finite = 1;
    rc = scal_features_create(&fc, &f);
    if (n < 1 && rc != SCAL_E_NO_DEVICE) {
        printf("expected SCAL_E_NO_DEVICE without a GPU, got %d (%s)\n", rc, scal_last_error());
        return 1;
    }
    if (rc == SCAL_OK) scal_features_destroy(f);
    memset(&pc, 0, sizeof pc);
    pc.lidar_type = SCAL_HDL64, pc.n_scans = 64, pc.minimum_range = 5.0, pc.max_points = 1000, pc.line_res = 0.4f, pc.plane_res = 0.8f;
    pc.max_map_points = 100000, pc.ring = 99;
    if (scal_pipeline_create(&pc, &p) != SCAL_E_ARG) { /* argument validation comes before any device work */
        printf("scal_pipeline_create accepted ring = 99\n");
        return 1;
    }
    memset(&rc_cfg, 0, sizeof rc_cfg);
    rc_cfg.max_corr_dist = 2.0, rc_cfg.transformation_epsilon = 1e-6, rc_cfg.fitness_epsilon = 1e-6, rc_cfg.fitness_gate = 0.3;
    rc_cfg.max_iterations = 100, rc_cfg.max_frames = 0, rc_cfg.max_points = 1000;
    if (scal_refine_create(&rc_cfg, &rf) != SCAL_E_ARG) {
        printf("scal_refine_create accepted max_frames = 0\n");
        return 1;
    }
    rc_cfg.max_frames = 4;
    rc = scal_refine_create(&rc_cfg, &rf);
    if (n < 1 && rc != SCAL_E_NO_DEVICE) {
        printf("scal_refine_create: expected SCAL_E_NO_DEVICE without a GPU, got %d (%s)\n", rc, scal_last_error());
        return 1;
    }
    if (rc == SCAL_OK) scal_refine_destroy(rf);
    memset(&rl_cfg, 0, sizeof rl_cfg); /* zero = the reference's default in every field but the capacities */
    rl_cfg.max_keyframes = 4, rl_cfg.max_points = 1000;
    if (scal_reloc_create(&rl_cfg, &rl) != SCAL_E_ARG) {
        printf("scal_reloc_create accepted max_query_points = 0\n");
        return 1;
    }
    rl_cfg.max_query_points = 1000;
    rc = scal_reloc_create(&rl_cfg, &rl);
    if (n < 1 && rc != SCAL_E_NO_DEVICE) {
        printf("scal_reloc_create: expected SCAL_E_NO_DEVICE without a GPU, got %d (%s)\n", rc, scal_last_error());
        return 1;
    }
    if (rc == SCAL_OK) {
        if (scal_reloc_size(rl) != 0 || !scal_reloc_sc(rl)) {
            printf("scal_reloc_create: a fresh context must be empty and own a ScanContext database\n");
            return 1;
        }
        scal_reloc_destroy(rl);
    }
    memset(&nb_cfg, 0, sizeof nb_cfg);
    nb_cfg.max_index_points = 1000;
    if (scal_nbr_create(&nb_cfg, &nb) != SCAL_E_ARG) {
        printf("scal_nbr_create accepted max_query_points = 0\n");
        return 1;
    }
    nb_cfg.max_query_points = 1000;
    rc = scal_nbr_create(&nb_cfg, &nb);
    if (n < 1 && rc != SCAL_E_NO_DEVICE) {
        printf("scal_nbr_create: expected SCAL_E_NO_DEVICE without a GPU, got %d (%s)\n", rc, scal_last_error());
        return 1;
    }
    if (rc == SCAL_OK) scal_nbr_destroy(nb);
    if (scal_nbr_knn_self(NULL, SCAL_NBR_MAX_K, NULL, NULL) != SCAL_E_ARG) {
        printf("scal_nbr_knn_self accepted a NULL context\n");
        return 1;
    }
    if (scal_nbr_normals_self(NULL, SCAL_NBR_MAX_K, NULL, NULL, NULL) != SCAL_E_ARG || scal_nbr_normals(NULL, NULL, 0, 3, NULL, NULL, NULL) != SCAL_E_ARG ||
        scal_nbr_normals_device(NULL, NULL, 0, 3, NULL, NULL, NULL) != SCAL_E_ARG || SCAL_NBR_NAN_BITS != 0x7fc00000u) {
        printf("scal_nbr_normals* accepted a NULL context\n");
        return 1;
    }
    printf("abi ok %s devices=%d\n", scal_version(), n);
    return 0;
}
