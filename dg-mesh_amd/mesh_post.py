"""The post-processing of an exported mesh, in the one order every export uses: clean, smooth, simplify, repair.

  clean     (mesh_clean)     drops the components that fail the criteria, invalid faces and unused vertices
  smooth    (mesh_smooth)    Taubin or Laplacian smoothing of the grid's staircase noise; faces stay
  simplify  (mesh_simplify)  quadric vertex clustering
  repair    (mesh_repair)    every body oriented consistently and outwards, small holes filled

Why this order: floaters go first, so that no later stage spends time on them or measures its box by them; the mesh is denoised
BEFORE it is decimated, because vertex clustering keeps the staircase it is given; and repair comes LAST, because clustering is what
opens and misorients a mesh -- it welds neighbouring sheets, drops the faces that collapse and can flip a triangle.

Per-vertex attributes (the exports' vertex colours; None stays None) follow their vertices: clean gathers the survivors' rows,
smooth passes them through, simplify gives a new vertex the row of its cluster's representative, repair appends to every attribute
the mean of its rim's rows for each vertex it adds.

The exports (MeshPhase.extract_mesh, evaluate.testing, visualize.export_dynamic_mesh, correspondence.export_correspondence) call
apply() and nothing else; a texture (mesh_texture) is baked on what apply() returns.  A new stage gets its module's apply(spec, verts,
faces, *attributes), a name in ORDER and a keyword here."""
import importlib

ORDER = ("clean", "smooth", "simplify", "repair")


def apply(verts, faces, *attributes, clean=None, smooth=None, simplify=None, repair=None):
    """-> (verts', faces', *attributes'): the four stages' own apply(), in ORDER.  Each spec is None, the stage's *Spec or a dict of
    its fields (the stage's as_spec); a stage whose spec is None is not imported or called, and with all four None the inputs
    themselves come back."""
    out = (verts, faces) + attributes
    for stage, spec in zip(ORDER, (clean, smooth, simplify, repair)):
        if spec is not None:
            out = importlib.import_module(f".mesh_{stage}", __package__).apply(spec, *out)
    return out
