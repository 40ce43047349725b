"""Knowledge distillation for the native T5: a teacher MyModel's logits for a student's loss forward.

    student.set_loss_options(distill_alpha=0.5, distill_temperature=2.0)
    t = distill.teacher_logits(teacher, images, source_encoding, target_encoding)
    loss = student(images, source_encoding, dict(target_encoding, teacher_logits=t))

Teacher and student are two MyModels with their own engines and workspaces; nothing is shared.  The tensor returned is a view of
the TEACHER's logits buffer (MyModel.logits): the student reads it in place, so it stays valid as long as the teacher runs no
other forward, generate or score before the student's forward has been issued -- clone it to keep it longer."""
import torch


def teacher_logits(teacher, images, source_encoding, target_encoding, student=None):
    """The teacher's logits for the labels of `target_encoding`: [B, Lt, V] ([B, n, Lt, V] for labels [B, n, Lt]) in the teacher's
    compute dtype, a view valid until the teacher's next forward, generate or score.  The teacher sees the same labels as the student,
    so its decoder inputs and the order of its rows are the student's.  Runs the teacher's loss forward in evaluation mode (restored
    afterwards) under torch.no_grad() with the plain loss options; loss weights and teacher logits in `target_encoding` are ignored.
    A teacher over another vocabulary is out of scope: with `student` given it raises here, before the teacher runs; otherwise the
    student's forward refuses the tensor by its shape."""
    if student is not None and teacher.main_cfg.vocab_size != student.main_cfg.vocab_size:
        raise ValueError(f"the teacher's vocab_size is {teacher.main_cfg.vocab_size}, the student's {student.main_cfg.vocab_size}: "
                         "distillation needs logits over one vocabulary")
    was_training = teacher.transformer.training
    saved = (dict(teacher._loss_options), dict(teacher._distill_options), teacher._weight_norm)
    teacher.transformer.eval()
    try:
        teacher.set_loss_options()
        with torch.no_grad():
            teacher(images, source_encoding, {"input_ids": target_encoding["input_ids"]})
        return teacher.logits()
    finally:
        teacher._loss_options, teacher._distill_options, teacher._weight_norm = saved
        teacher.transformer.train(was_training)

