/* Host-side scene-graph loader, second header: GQA object ids -> node indices of the converted graphs.
 *
 * GQA's question records carry `annotations`: word positions of the question, the answer and the full answer mapped to the id
 * of the scene-graph object the words refer to.  The conversion numbers an image's nodes by the ascending order of the object id
 * STRINGS (std::string order, so "10" < "9"; ISubGVQA/datasets/scene_graph.py:233-236); the store keeps those strings, in node
 * order, in one pool for all images, and this header resolves ids against them.
 *
 * Same library (libisg_loader.so) and conventions as include/isg_loader.h: status codes ISG_LD_*, isg_sg_last_error() for the
 * text, nothing throws.  An ABI version of its own: isg_loader.h does not move when an entry point here does.
 */
#ifndef ISG_LOADER_OBJECTS_H
#define ISG_LOADER_OBJECTS_H

#include <stdint.h>

#include "isg_loader.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISG_LOADER_OBJECTS_ABI_VERSION 1

#define ISG_LD_NO_NODE (-2)   /* the object is not a node of the graph a collate of that image gives */

int isg_loader_objects_abi_version(void);

/* For B questions: slots int64 [B] (isg_sg_store_find_many's; -1 = the image is not in the store), id_ptr int64 [B + 1] ascending
 * from 0, object_ids id_ptr[B] C strings (question b asks for object_ids[id_ptr[b] .. id_ptr[b + 1])), nodes int32 [id_ptr[B]].
 * nodes[i] = the LOCAL node index of that object in that image's graph, or ISG_LD_NO_NODE where the image is absent, where the
 * image's graph is a dummy (an image without objects, and an image whose graph is a single self loop, which every collate
 * replaces by the 6-node dummy: nothing resolves against a dummy), where the image has no such object, and for a NULL string.
 * ISG_LD_EINVAL: a NULL store, B < 0, a NULL slots / id_ptr with B > 0, id_ptr[0] != 0 or descending, a NULL object_ids / nodes with
 * id_ptr[B] > 0. */
int isg_sg_store_object_nodes(const isg_sg_store *s, const int64_t *slots, int64_t B, const int64_t *id_ptr,
                              const char *const *object_ids, int32_t *nodes);

/* Bytes the store holds for this: the characters of the id pool plus one int64 offset per object and one per image; -1 for a
 * NULL store. */
int64_t isg_sg_store_object_bytes(const isg_sg_store *s);

#ifdef __cplusplus
}
#endif
#endif
